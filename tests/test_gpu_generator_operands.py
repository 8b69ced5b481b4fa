"""The beta-CEM generators' operands, bit for bit against the build that stored
them: beta-iterations 0..2 through the stage API, then the whole risk stage
(tests/generator_operands.py has the walk), against arrays recorded from the
parent commit's build (tests/golden/generator_operands/, recorded by
tests/golden/make_generator_operands_golden.py, which names the commit).

That build's k_belite wrote the U rows of the generators (u_e = (E_e - m) /
sqrt(10), the fp32-rounded mean in slot 11) as a second fp64 plane of ``gen``,
read back by k_bgen / k_bgen_wave, k_bsigma, the samplers and k_bcem_small;
now every reader forms them from the elite rows (``belite``) and the fp64
means with one helper (layout.hpp: gen_u), and the samplers stop at the last
block that holds a position.  Neither may move a bit of: the W plane of
``gen``, ``genm``, ``phib``, the real rows of ``ygen``, ``belite`` (first two
candidates), nor of beta / sigma / res_beta after the whole stage.

Shapes: n = 6, 12, 22 (block counts 3 + 1 padding, 10 with a last block that
holds the sigma coordinate alone, 31 + 1 padding; 1, 2, 4 chunks), each on a
384-candidate handle (k_bsample's one-wave walker; MPCMMD_GENWAVE=0 pins the
quad k_bgen that handles above 512 candidates take) and on a 20-candidate
one -- the smallest num_batch a handle accepts -- (k_bsample_chunks,
k_bgen_wave; k_bcem_small in stage 2 at n = 6 and 12)."""
import os

import numpy as np
import pytest

import generator_operands as go

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generator_operands")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


@pytest.mark.parametrize("n,B,genwave", go.CASES, ids=[go.case_id(n, B) for n, B, _ in go.CASES])
def test_generator_operands_bits(native, monkeypatch, n, B, genwave):
    for k in ("MPCMMD_GENWAVE", "MPCMMD_FUSED", "MPCMMD_GROUPS"):
        monkeypatch.delenv(k, raising=False)
    if genwave is not None:
        monkeypatch.setenv("MPCMMD_GENWAVE", genwave)
    steps, info = go.walk(native, n, B)
    # which kernels ran: the generator variant, and in stage 2 the fused kernel
    # exactly where bcem_small_ok takes the handle (gen_wave, M <= 256, <= 512 candidates)
    assert info["gen_wave"] == (0 if genwave == "0" else 1)
    assert info["fused_small"] == 1
    fused = info["gen_wave"] == 1 and n * n <= 256 and B <= 512
    assert fused == (B == 20 and n in (6, 12))
    bad = []
    for step, arrays in steps.items():
        with np.load(os.path.join(GOLDEN, f"{go.case_id(n, B)}_{step}.npz")) as ref:
            assert int(ref["gen_wave"]) == info["gen_wave"], "fixture recorded with the other generator kernel"
            for k, a in arrays.items():
                r = ref[k]
                assert a.shape == r.shape and a.dtype == r.dtype, f"{step} {k}: {a.shape} {a.dtype} / {r.shape} {r.dtype}"
                d = _bits(a) != _bits(r)
                print(f"{go.case_id(n, B)} {step} {k}: {int(d.sum())} of {d.size} words differ")
                if d.any():
                    bad.append(f"{step} {k}: {int(d.sum())} of {d.size} words differ, first at {np.argwhere(d)[0].tolist()}")
    assert not bad, "; ".join(bad)
