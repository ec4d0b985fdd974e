"""The hoisted Philox call of the ELBO scan against the plain one, on the host.

`pf_philox_draw_invariants`, `pf_philox_block_product` and `pf_philox4x32_hoisted` (pathfinder.jl_amd/csrc/pfmi_common.h) split a
Philox4x32 call with counter (n, g, 0, 0) into what depends on the draw, on the row group, and on both.  They are `__host__ __device__`
and integer only, so a host program sees the words the kernel sees.  tests/host/philox_hoist_check.hip compares them with
`pf_philox4x32<PF_NORMAL_ROUNDS>` word for word: every (n, g, k0, k1) over {0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF}, keys for which
k + j W wraps at every round, and 10^5 seeded random tuples (twice: full range, and the scan's small draw / row-group indices).  The
program makes no HIP call and needs no GPU.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "tests", "host", "philox_hoist_check.hip")


def _build(out, extra=()):
    cmd = [HIPCC, "--cuda-host-only", "-std=c++17", "-O1", *extra, "-I", os.path.join(ROOT, "pathfinder.jl_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), SRC, "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


@pytest.mark.parametrize("flags", [(), ("-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "ubsan"])
def test_hoisted_call_gives_the_same_words(tmp_path, flags):
    exe = str(tmp_path / "philox_hoist_check")
    _build(exe, flags)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 200000, r.stdout
