"""Which of rt_solver's options are not supported together is one table in csrc/rt_solver_options.hpp, and every refusal's message is
made from it.  tests/solver_options_host.cpp checks the table, the messages and — pair by pair — that plan_sweep (rt_sweep_plan.hpp)
refuses what the table lists; here the program is built without sanitizers and run (tests/sanitize/run.sh builds it with
AddressSanitizer + UBSan).  No GPU, no HIP header."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solver_options_on_the_host(tmp_path):
    exe = tmp_path / "solver_options"
    src = os.path.join(ROOT, "tests", "solver_options_host.cpp")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-o", str(exe), src])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"solver_options: (\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) > 100000, r.stdout


def test_options_header_is_host_only():
    """The header compiles as plain C++ and names no HIP header and no other header of the library."""
    hdr = os.path.join(ROOT, "raytracing.jl_amd", "csrc", "rt_solver_options.hpp")
    text = open(hdr, encoding="utf-8").read()
    includes = re.findall(r'#include [<"]([^>"]+)[>"]', text)
    assert includes and not [i for i in includes if "hip" in i.lower() or i.startswith("rt_")], includes


def test_solver_names_no_pair_itself():
    """No solver source file (rt_solver.hip, rt_solver_set.hip, rt_solver_state.hpp: every rt_solver* under csrc/ but the table itself)
    holds text of its own that names two options as unsupported together: the table's formatters make them all."""
    csrc = os.path.join(ROOT, "raytracing.jl_amd", "csrc")
    names = sorted(f for f in os.listdir(csrc) if f.startswith("rt_solver") and f != "rt_solver_options.hpp")
    assert {"rt_solver.hip", "rt_solver_set.hip", "rt_solver_state.hpp"} <= set(names), names
    for name in names:
        text = open(os.path.join(csrc, name), encoding="utf-8").read()
        assert not re.findall(r'"[^"\n]*(?:together with|the two together)[^"\n]*"', text), name
        assert "pn_refuses" not in text and "krylov_conflict" not in text, name
