"""MI355X-native ``segmentize!`` for RayTracing.jl-style cyclic ray tracing.

Host-side mirror of the reference's public surface (``src/RayTracing.jl:32-35``):
``BoundaryConditions, Vacuum, Reflective, Periodic, TrackGenerator, trace!, segmentize!``
(Python spells the last two ``trace`` and ``segmentize``).  ``segmentize`` runs the
hand-written HIP kernels in ``csrc/`` through the C ABI declared in
``include/rt_segmentize.h``; there is no CPU fallback — without the built library or
without a GPU it raises.  ``solve_eigenvalue`` / ``solve_fixed_source`` run a MOC
source iteration on the device over the records of the last ``segmentize``, forward or
adjoint; ``perturbation_reactivity`` / ``kinetics_parameters`` weigh with the adjoint flux.
``SolverBoundary`` puts albedos and an incoming flux on the four sides and makes a run
return the partial currents per side and the neutron balance.  ``solve_transient`` continues
an eigenvalue result in time with ``Kinetics`` data (implicit Euler, delayed neutrons).
"""
from .boundary import BoundaryConditions, BoundaryType, Periodic, Reflective, Vacuum
from .mesh import DiscreteModel, DiscreteModelFromFile, GmshDiscreteModel, Mesh, data_path
from .quadrature import AzimuthalQuadrature
from .trackgenerator import (Backward, Forward, Segment, Track, TrackGenerator, bc_bwd, bc_fwd,
                             dir_next_track_bwd, dir_next_track_fwd, trace, track_end_sides)
from .segmentize import RTOL_DEFAULT, SegmentStore, segmentize
from .solver import (Cmfd, CrossSections, PolarQuadrature, SolverBoundary, SolverResult, azimuthal_weights, exact_azimuthal_weights, diffusion_coupling,
                     kinetics_parameters, perturbation_reactivity, solve_eigenvalue, solve_fixed_source, Kinetics, TransientResult, solve_transient, Krylov)
from .distributed import ShardedSolver
from ._capi import DeviceMesh, DeviceSolver  # point location and flux sampling: Mesh.find_elements / locate_grid, DeviceSolver.sample

__all__ = [
    "BoundaryConditions", "BoundaryType", "Vacuum", "Reflective", "Periodic",
    "DiscreteModel", "DiscreteModelFromFile", "GmshDiscreteModel", "Mesh", "data_path",
    "AzimuthalQuadrature", "TrackGenerator", "trace", "segmentize", "SegmentStore", "RTOL_DEFAULT",
    "Track", "Segment",
    "CrossSections", "PolarQuadrature", "SolverResult", "azimuthal_weights", "exact_azimuthal_weights",
    "solve_eigenvalue", "solve_fixed_source", "perturbation_reactivity", "kinetics_parameters", "ShardedSolver",
    "SolverBoundary", "track_end_sides", "Cmfd", "diffusion_coupling", "Kinetics", "TransientResult", "solve_transient", "Krylov",
    "DeviceMesh", "DeviceSolver",
    "Forward", "Backward", "bc_fwd", "bc_bwd", "dir_next_track_fwd", "dir_next_track_bwd",
]
