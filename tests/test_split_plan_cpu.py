"""The split plan of a track set (pieces per wave of 64 uids, canonical numbering, dispatch order) is plan_split in
csrc/rt_hostpar.hpp.  tests/sanitize/hostpar_san.cpp checks it — the plan's properties at the sizes where the rule turns, in the three
modes of the option, and three plans worked by hand — under the sanitizers (tests/sanitize/run.sh); here the same checks are built
without them and run alone.  No GPU, no HIP header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_plan_on_the_host(tmp_path):
    exe = tmp_path / "hostpar"
    src = os.path.join(ROOT, "tests", "sanitize", "hostpar_san.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", "-o", str(exe), src])
    r = subprocess.run([str(exe), "split"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hostpar_san: split plans (6 sizes x 3 modes x 2 caps, 3 by hand): ok" in r.stdout, r.stdout + r.stderr
