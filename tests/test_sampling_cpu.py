"""The host side of the seeded fused sampler (ullsam_sample_topk_topp): the Philox mirror against Random123's known answers, the seed / uniform
mappings, the entry point's declaration against its binding and the built library, and the float64 definition the GPU tests check the kernel with
(tests/sampling_ref.py) against the repository's own torch sampling route on tie-free rows."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import sampling_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("counter,key,want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(counter, key, want):
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    from ullsam_amd import sampling
    out = sampling.philox4x32_10(counter, key)
    assert out.dtype == np.uint32 and out.shape == (4,)
    assert _hex(out) == want
    both = sampling.philox4x32_10(np.array([counter, [0, 0, 0, 0]]), np.array([key, [0, 0]]))     # batched: the same words
    assert _hex(both[0]) == want and _hex(both[1]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"


def test_uniforms_and_row_seeds():
    from ullsam_amd import sampling
    seeds = np.array([0, 1, 2 ** 32, 2 ** 64 - 1, 12345678901234567], dtype=np.uint64)
    seen = set()
    for step in (0, 1, 2, 2 ** 32 + 5):
        u = sampling.uniforms(seeds, step)
        assert u.dtype == np.float32 and u.shape == (5,)
        assert bool(((u >= 0) & (u < 1)).all())
        scaled = u.astype(np.float64) * 2.0 ** 24
        assert bool((scaled == np.round(scaled)).all())                      # multiples of 2^-24
        for b, s in enumerate(seeds):                                        # exactly the stated mapping
            w0 = sampling.philox4x32_10([step & 0xFFFFFFFF, step >> 32, 0, 0], [int(s) & 0xFFFFFFFF, int(s) >> 32])[0]
            assert float(u[b]) == (int(w0) >> 8) * 2.0 ** -24
        seen.update((step, int(s), float(v)) for s, v in zip(seeds, u))
    assert len({v for _, _, v in seen}) == len(seen) == 20                   # differ across seeds and steps
    s = 2 ** 40 + 17
    assert sampling.row_seeds(s, 3).tolist() == [s, s + 1, s + 2]
    assert sampling.row_seeds(s, 3).dtype == np.uint64
    assert sampling.row_seeds(2 ** 64 - 1, 2).tolist() == [2 ** 64 - 1, 0]   # mod 2^64
    assert sampling.row_seeds([7, 3, 9], 3).tolist() == [7, 3, 9]
    with pytest.raises(ValueError):
        sampling.row_seeds([1, 2], 3)


def test_entry_is_declared_bound_and_exported():
    from ullsam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+ullsam_sample_topk_topp\s*\(([^;]*)\)\s*;", hdr)
    assert m, "ullsam_sample_topk_topp is not declared in include/ullsam_hip.h"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    assert n_args == len(_lib.SIGNATURES["ullsam_sample_topk_topp"]) == 15
    lib = ctypes.CDLL(_lib.LIB_PATH) if os.path.exists(_lib.LIB_PATH) else None
    assert lib is not None, "build the library first (python -m ullsam_amd.build)"
    assert hasattr(lib, "ullsam_sample_topk_topp")


@pytest.mark.parametrize("T,k,p", [(0.7, 50, 0.9), (1.3, 5, 0.5), (1.0, 64, None)])
def test_reference_agrees_with_the_torch_route_as_a_distribution(T, k, p):
    """On tie-free rows the float64 definition and _sampling_probs (the route generate takes without a seed) are the same distribution: max abs
    difference < 1e-5 over the vocabulary (fp32 softmax against float64; a nucleus boundary closer than that to a cumulative mass would differ by a
    whole probability, so the rows are checked to have none)."""
    from ullsam_amd.modeling.modeling_internlm2 import _sampling_probs
    g = torch.Generator(); g.manual_seed(int(T * 10) + k)
    x = torch.randn((4, 3001), generator=g) * 3.0
    x[1, 77] += 9.0                                                          # a peaked row: the nucleus is a token or two
    got = _sampling_probs(x, T, k, p).double().numpy()
    for r in range(x.shape[0]):
        row = x[r].numpy()
        assert len(np.unique(np.sort(row)[-(k + 1):])) == k + 1              # tie-free where it matters: the k largest and the one they end at
        ref = R.reference(row, T, k, p)
        if p is not None:
            assert np.abs(ref["before"][1:] - p).min() > 1e-4
        want = np.zeros(row.size)
        want[ref["ids"]] = ref["probs"]
        assert abs(want.sum() - 1.0) < 1e-12
        assert np.abs(got[r] - want).max() < 1e-5


def test_reference_helper_edges():
    """The helper's own edges: ties go to the lower id, NaN counts as -inf, +inf and empty rows put all mass on candidate 0, accepted() is the token
    of u's interval away from the boundaries and both neighbours at one."""
    row = np.array([1.0, 2.0, 2.0, np.nan, 2.0, -np.inf, 0.5], np.float32)
    ref = R.reference(row, 1.0, 3, None)
    assert ref["ids"].tolist() == [1, 2, 4] and np.allclose(ref["probs"], 1 / 3)
    assert R.reference(row, 1.0, 7, None)["ids"].tolist() == [1, 2, 4, 0, 6, 3, 5]
    inf = R.reference(np.array([0.0, np.inf, 3.0, np.inf], np.float32), 0.7, 3, 0.9)
    assert inf["ids"].tolist() == [1, 3, 2] and inf["probs"].tolist() == [1.0, 0.0, 0.0]
    empty = R.reference(np.array([np.nan, -np.inf, np.nan], np.float32), 0.7, 2, 0.9)
    assert empty["ids"].tolist() == [0, 1] and empty["probs"].tolist() == [1.0, 0.0]
    ref = R.reference(np.log(np.array([0.5, 0.25, 0.125, 0.125])), 1.0, 4, 0.8)      # masses before: 0, .5, .75, .875 -> the last one goes
    assert np.allclose(ref["probs"], [4 / 7, 2 / 7, 1 / 7, 0.0])
    eps = R.eps_for(4)
    assert R.accepted(ref, 0.3, eps) == {0} and R.accepted(ref, 0.99, eps) == {2}
    assert R.accepted(ref, 4 / 7, eps) == {0, 1}
    edge = R.reference(np.log(np.array([0.5, 0.25, 0.25])), 1.0, 3, 0.75)              # the third candidate sits on the boundary: kept or dropped
    assert R.accepted(edge, 0.7, R.eps_for(3)) == {1}
    assert R.accepted(edge, 0.9, R.eps_for(3)) == {1, 2}
