"""csrc/dw_plan.h on the host: the dW GEMM's plan — the 64x64 block list, the split kernel's passes (matrices grouped, large ones cut into chunks of
output blocks, first-fit bins) and the slice count — for the networks the engines run: 3 x (96-50-20-31), fc32 at Nz = 32 and 64, 3 x (96-400-400-31),
32-128-128-31 and 64-256-256-63.  tests/dw_plan_check.cpp asserts the planner's invariants itself (every block in exactly one pass; at most 16 blocks,
768 compact features and 8 segments per pass; maxm and nit as derived from the pass; compacted features inside their segment; the slice rule for 1, 12
and 4,096 records with and without LDS fit) and prints every plan; the text must equal tests/golden/dw_plan_parent.txt, value for value — the plans of
the code this header replaced (tests/golden/dw_plan_parent.md says how they were recorded).  No GPU, no library, no preload.

The program is compiled host-only with hipcc, not g++: DevModel and DwMacro live in colnde_dev.h, which includes the HIP headers (and device builtins).
Nothing in it calls HIP."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NETS = ["3x96-50-20-31", "fc32_Nz32", "fc32_Nz64", "3x96-400-400-31", "32-128-128-31", "64-256-256-63"]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dw_plan") / "dw_plan_check")
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1",
                           os.path.join(ROOT, "tests", "dw_plan_check.cpp"), "-I", os.path.join(ROOT, "climateparameterizations.jl_amd", "csrc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr                   # an invariant of the planner failed: stderr names the network and the line
    return _by_net(r.stdout)


def _by_net(text):
    out, name = {}, None
    for ln in text.splitlines():
        if ln.startswith("net "):
            name = ln.split()[1]
            assert name not in out
            out[name] = []
        out[name].append(ln)
    return out


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(ROOT, "tests", "golden", "dw_plan_parent.txt")) as f:
        return _by_net(f.read())


def test_the_program_walks_every_network(plans, parent):
    assert list(plans) == NETS and list(parent) == NETS


@pytest.mark.parametrize("net", NETS)
def test_plan_equals_the_parents_value_for_value(plans, parent, net):
    got, want = plans[net], parent[net]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (net, i)
    assert len(got) == len(want)
    # the fixture is a whole plan: blocks, passes with their segments, the compacted list, 3 record counts x LDS fit x arithmetic
    n_mac = int(want[0].split()[-1])
    assert sum(ln.startswith("mac ") for ln in want) == n_mac == sum(ln.startswith("smac ") for ln in want) and want[n_mac + 1].startswith("split_ok 1 ")
    assert sum(ln.startswith("slices ") for ln in want) == 12


def test_the_wide_matrices_are_cut_into_chunks(parent):
    """3 x (96-400-400-31): a 400 x 400 matrix has 49 blocks and 800 operand features, more than a pass holds — its blocks are spread over several passes."""
    passes = [ln.split() for ln in parent["3x96-400-400-31"] if ln.startswith("pass ")]
    assert len(passes) == 18 and sum(int(p[9]) for p in passes) == 210 and max(int(p[9]) for p in passes) <= 16
