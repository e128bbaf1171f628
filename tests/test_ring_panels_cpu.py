"""The ring GEMM's K-panel weight layout (ullsam_amd.packing.pack_ring_panels, csrc/gemm_ring8p.h) on the host: the index formula, the round trip,
the refusals, the SwiGLU pack underneath it, and the header's declarations of the entry points that carry both weight pointers."""
import os
import re

import pytest
import torch

from ullsam_amd import _lib
from ullsam_amd.packing import pack_ring_panels, pack_w13, unpack_ring_panels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _weight(N, K, seed):
    g = torch.Generator(); g.manual_seed(seed)
    return torch.randn(N, K, generator=g).bfloat16()


def _by_formula(w):
    """Row R, element k of [N, K] -> flat index ((R // 16) (K // 32) + k // 32) 512 + (R % 16) 32 + k % 32, as a plain loop."""
    N, K = w.shape
    flat = [None] * (N * K)
    src = w.view(torch.int16).tolist()
    for R in range(N):
        for k in range(K):
            flat[((R // 16) * (K // 32) + k // 32) * 512 + (R % 16) * 32 + k % 32] = src[R][k]
    assert all(v is not None for v in flat)
    return torch.tensor(flat, dtype=torch.int16)


@pytest.mark.parametrize("N,K", [(32, 64), (272, 128)])
def test_pack_ring_panels_is_the_index_formula(N, K):
    w = _weight(N, K, N + K)
    p = pack_ring_panels(w)
    assert p.shape == w.shape and p.dtype == torch.bfloat16 and p.is_contiguous()
    assert p.data_ptr() % 1024 == 0                      # a cell is one ALIGNED KiB
    assert torch.equal(p.reshape(-1).view(torch.int16), _by_formula(w))
    # the same as the one-line statement of the layout
    assert torch.equal(p.reshape(-1), w.view(N // 16, 16, K // 32, 32).permute(0, 2, 1, 3).contiguous().reshape(-1))
    # one (16-row block, k step) cell = 16 rows x 32 k, contiguous
    cell = p.reshape(-1)[(1 * (K // 32) + 1) * 512:(1 * (K // 32) + 1) * 512 + 512].view(16, 32)
    assert torch.equal(cell, w[16:32, 32:64])


@pytest.mark.parametrize("N,K", [(32, 64), (272, 128), (16, 32)])
def test_pack_ring_panels_round_trip(N, K):
    w = _weight(N, K, 7 * N + K)
    assert torch.equal(unpack_ring_panels(pack_ring_panels(w)), w)
    v = _weight(N, 2 * K, 3)[:, :K]                      # a strided view packs like its contiguous copy
    assert torch.equal(pack_ring_panels(v), pack_ring_panels(v.contiguous()))


@pytest.mark.parametrize("N,K,dtype", [(24, 64, torch.bfloat16), (32, 48, torch.bfloat16), (32, 64, torch.float32)])
def test_pack_ring_panels_refuses_other_shapes(N, K, dtype):
    with pytest.raises(ValueError):
        pack_ring_panels(torch.zeros(N, K, dtype=dtype))


def test_pack_w13_then_panels_is_the_formula_on_the_interleaved_rows():
    I, K = 128, 64
    w1, w3 = _weight(I, K, 1), _weight(I, K, 2)
    rows = torch.empty(2 * I, K, dtype=torch.bfloat16)   # alternating 64-row blocks (gate block t, up block t), written out
    for t in range(I // 64):
        rows[128 * t:128 * t + 64] = w1[64 * t:64 * t + 64]
        rows[128 * t + 64:128 * t + 128] = w3[64 * t:64 * t + 64]
    w13 = pack_w13(w1, w3)
    assert torch.equal(w13, rows)
    assert torch.equal(pack_ring_panels(w13).reshape(-1).view(torch.int16), _by_formula(rows))


def _header_arity(name):
    src = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
    assert m, f"{name} is not declared in include/ullsam_hip.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name,base", [("ullsam_gemm_panels", "ullsam_gemm"), ("ullsam_gemm_qkv_rope_panels", "ullsam_gemm_qkv_rope")])
def test_header_declares_the_panel_entry_points(name, base):
    assert _header_arity(name) == len(_lib.SIGNATURES[name])
    assert _header_arity(name) == _header_arity(base) + 1 == len(_lib.SIGNATURES[base]) + 1     # the same call plus the second weight pointer ...
    sig, bsig = _lib.SIGNATURES[name], _lib.SIGNATURES[base]
    assert sig[:5] == bsig[:5] and sig[5] == _lib.vp and sig[6:] == bsig[5:]                    # ... right behind (W, ldw)
    src = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    assert re.search(r"#define\s+ULLSAM_ABI_VERSION\s+14\b", src)                               # an added export leaves the version alone
