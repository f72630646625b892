"""What one rt_sweep call decides — the rows it reads, the passes' width, LDS copy and launch shape, its refusals — is a pure
function in csrc/rt_sweep_plan.hpp.  tests/sanitize/sweep_plan_san.cpp checks it on the host against the values sweep_impl computed
when the decisions still lived in it, and that every pass of a plan it does not refuse has a kernel (pass_kernel_key); here the program is built without sanitizers and run (tests/sanitize/run.sh builds it with
AddressSanitizer + UBSan).  No GPU, no HIP header."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_plan_on_the_host(tmp_path):
    exe = tmp_path / "sweep_plan"
    src = os.path.join(ROOT, "tests", "sanitize", "sweep_plan_san.cpp")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-o", str(exe), src])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"sweep_plan_san: (\d+) checks, 0 failed", r.stdout)
    assert m and int(m.group(1)) > 500, r.stdout


def test_plan_header_is_host_only():
    """The header compiles as plain C++ and names no HIP header: the sweep's decisions can be checked where there is no GPU."""
    hdr = os.path.join(ROOT, "raytracing.jl_amd", "csrc", "rt_sweep_plan.hpp")
    text = open(hdr, encoding="utf-8").read()
    includes = re.findall(r'#include [<"]([^>"]+)[>"]', text)
    assert includes and not [i for i in includes if "hip" in i.lower() or i.startswith("rt_")], includes
