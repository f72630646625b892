"""A mesh handle's options (rt_set_option) are one struct and one table of name / member / rule in csrc/rt_mesh_options.hpp.
tests/mesh_options_host.cpp probes every option with the same nine values against the rule of its group, the refusals' exact texts,
that a refused call changes nothing, and the defaults; here the program is built and run.  No GPU, no HIP header."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing.jl_amd", "csrc")


def test_mesh_options_on_the_host(tmp_path):
    exe = tmp_path / "mesh_options"
    src = os.path.join(ROOT, "tests", "mesh_options_host.cpp")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-o", str(exe), src])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"mesh_options: (\d+) checks, 0 failed", r.stdout)
    # nine probes of 33 options, three checks each, and the refusals
    assert m and int(m.group(1)) > 9 * 33 * 3, r.stdout


def test_options_header_is_host_only():
    """The header compiles as plain C++ and names no HIP header and no other header of the library."""
    text = open(os.path.join(CSRC, "rt_mesh_options.hpp"), encoding="utf-8").read()
    includes = re.findall(r'#include [<"]([^>"]+)[>"]', text)
    assert includes and not [i for i in includes if "hip" in i.lower() or i.startswith("rt_")], includes


def test_no_option_chain_left():
    """No .hip file under csrc/ compares an option's name itself any more, except rt_set_option's one for "walk" (which touches the
    handle's state, not an option)."""
    found = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(".hip"):
            text = open(os.path.join(CSRC, name), encoding="utf-8").read()
            found += [(name, line.strip()) for line in text.splitlines() if "strcmp(name," in line]
    assert len(found) == 1 and found[0][0] == "rt_handles.hip" and 'strcmp(name, "walk")' in found[0][1], found
