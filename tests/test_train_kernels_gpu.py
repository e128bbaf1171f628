"""The training kernels of csrc/train.hip, one by one, against float64 definitions of the same operations at the shapes, layouts and edges where
their code paths divide (row blocks, LDS chunks, register instantiations, the MFMA threshold, 16-byte fetches, causal tile clipping), and the
attention autograd Function route by route against float64 autograd of the reference's softmax attention with its additive finfo.min masks
(modeling_internlm2.py:96-125, 830-851).  Every reference is computed here by torch in float64; nothing is read from fixtures.

Tolerances follow fp32 rounding: an fp32 result is held to at most 1e-5 of the scale of its reference (sums of n terms: 2e-6 max(1, sqrt(n) / 8)
of the scale, capped there); integer-valued inputs make the ordered sums exact, and there the kernels must match bit for bit.  bf16 products are
held to float64 products of their bf16-rounded operands; the bf16 attention routes to 1.5x torch's own autocast(bfloat16) error plus a floor."""
import contextlib
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMIN = torch.finfo(torch.float32).min


def _lib():
    from ullsam_amd import _lib as L
    return L


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _randn(shape, g, scale=1.0):
    return torch.randn(shape, device=DEV, generator=g, dtype=torch.float32) * scale


def _ints(shape, g, lo=-3, hi=4):
    return torch.randint(lo, hi, shape, device=DEV, generator=g).float()


def _err(a, ref):
    return float((a.double() - ref.double()).abs().max())


def _scale(ref):
    return max(float(ref.double().abs().max()), 1e-30)


def _tol(n=1):
    """fp32 rounding of a sum of n terms, relative to the scale of its result; never looser than 1e-5."""
    return min(1e-5, 2e-6 * max(1.0, math.sqrt(n) / 8))


def _close(a, ref, n=1, what=""):
    e, sc = _err(a, ref), _scale(ref)
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    assert e <= _tol(n) * sc, f"{what}: max err {e:.3e} > {_tol(n):.1e} x scale {sc:.3e}"


def _misaligned(t):
    """A copy of t whose base pointer is 4 bytes past a 16-byte boundary (forces the kernels' per-element forms)."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    off = next(o for o in range(4) if (buf.data_ptr() + 4 * o) % 16 == 4)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. elementwise kernels and ordered reductions
# ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [1, 2])
def test_act_forward_and_backward_against_float64(kind):
    """ullsam_train_act: exact GELU (kind 1) and ReLU (kind 2), y and dy * act'(x), over |x| <= 40 with x = 0 exactly and n not a multiple of 256."""
    g = _gen(kind)
    x = torch.cat([torch.linspace(-40, 40, 4001, device=DEV), torch.zeros(7, device=DEV), _randn((5003,), g, 3.0)]).contiguous()
    dy = _randn(x.shape, g)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    _lib().call("ullsam_train_act", x.data_ptr(), None, y.data_ptr(), x.numel(), kind, _s())
    _lib().call("ullsam_train_act", x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), kind, _s())
    xd, gd = x.double(), dy.double()
    if kind == 1:
        cdf = 0.5 * (1 + torch.erf(xd / math.sqrt(2)))
        ref_y, ref_dx = xd * cdf, gd * (cdf + xd * torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi))
        # elementwise: fp32 erf near the tails loses what 1 + erf cancels (a few 1e-8 absolute), scaled by |x|
        mag = xd.abs().clamp(min=1.0)
        assert bool(((y.double() - ref_y).abs() <= 1e-6 * mag).all()), _err(y, ref_y)
        assert bool(((dx.double() - ref_dx).abs() <= 1e-6 * mag * gd.abs().clamp(min=1.0)).all()), _err(dx, ref_dx)
        assert float(y[x == 0].abs().max()) == 0.0 and bool((dx[x == 0] == 0.5 * dy[x == 0]).all())
    else:
        assert torch.equal(y, torch.relu(x))
        assert torch.equal(dx, torch.where(x > 0, dy, torch.zeros_like(dy)))      # torch's threshold_backward: 0 at x == 0


def test_swiglu_forward_and_backward_against_float64():
    """ullsam_train_swiglu: silu(g) u and its gradients with |g| up to 90 (expf(-g) overflows to inf for g < -88: s = 0, no NaN)."""
    g0 = _gen(3)
    gv = torch.cat([torch.linspace(-90, 90, 1801, device=DEV), torch.zeros(3, device=DEV), _randn((3000,), g0, 4.0)]).contiguous()
    u, dy = _randn(gv.shape, g0), _randn(gv.shape, g0)
    out, dg, du = torch.empty_like(gv), torch.empty_like(gv), torch.empty_like(gv)
    _lib().call("ullsam_train_swiglu", gv.data_ptr(), u.data_ptr(), None, out.data_ptr(), None, None, gv.numel(), _s())
    _lib().call("ullsam_train_swiglu", gv.data_ptr(), u.data_ptr(), dy.data_ptr(), None, dg.data_ptr(), du.data_ptr(), gv.numel(), _s())
    gd = gv.double().requires_grad_(True)
    ud = u.double().requires_grad_(True)
    ref = F.silu(gd) * ud
    ref.backward(dy.double())
    for a, r, m in ((out, ref.detach(), gv.double().abs() * u.double().abs()), (dg, gd.grad, (1 + gv.double().abs()) * (u * dy).double().abs()),
                    (du, ud.grad, gv.double().abs() * dy.double().abs())):
        assert torch.isfinite(a).all()
        assert bool(((a.double() - r).abs() <= 1e-6 * (r.abs() + m + 1e-30)).all()), _err(a, r)


@pytest.mark.parametrize("n", [1, 63, 1023, 1025, 70000])
def test_scale_shift_forward_and_backward_against_float64(n):
    """ullsam_train_scale_shift: y = x s + t; dx = dy s, ds += sum dy x, dt += sum dy through per-1024 partials and the 64-lane ordered_sum_kernel
    (n up to 69 partials: some lanes sum two, some none).  Integer-valued inputs: the sums are exact and must match exactly."""
    g = _gen(n)
    for integer in (True, False):
        x, dy = (_ints((n,), g), _ints((n,), g)) if integer else (_randn((n,), g), _randn((n,), g))
        s, t = torch.tensor([1.5], device=DEV), torch.tensor([-0.25], device=DEV)
        y = torch.empty_like(x)
        _lib().call("ullsam_train_scale_shift", x.data_ptr(), s.data_ptr(), t.data_ptr(), None, y.data_ptr(), None, None, n, None, _s())
        dx = torch.empty_like(x)
        ds, dt = torch.tensor([0.5], device=DEV), torch.tensor([2.0], device=DEV)          # accumulated into
        part = torch.full((2 * -(-n // 1024),), float("nan"), device=DEV)
        _lib().call("ullsam_train_scale_shift", x.data_ptr(), s.data_ptr(), t.data_ptr(), dy.data_ptr(), dx.data_ptr(), ds.data_ptr(), dt.data_ptr(), n,
                    part.data_ptr(), _s())
        xd, gd = x.double(), dy.double()
        ref_ds, ref_dt = 0.5 + (gd * xd).sum(), 2.0 + gd.sum()
        if integer:
            assert torch.equal(y.double(), xd * 1.5 - 0.25) and torch.equal(dx.double(), gd * 1.5)
            assert float(ds) == float(ref_ds) and float(dt) == float(ref_dt), (float(ds), float(ref_ds), float(dt), float(ref_dt))
        else:
            _close(y, xd * 1.5 - 0.25, 1, "scale_shift y")
            _close(dx, gd * 1.5, 1, "scale_shift dx")
            assert abs(float(ds) - float(ref_ds)) <= _tol(n) * float((gd * xd).abs().sum())
            assert abs(float(dt) - float(ref_dt)) <= _tol(n) * float(gd.abs().sum())


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 4095, 4097, 70000])
def test_colsum_against_float64(rows):
    """ullsam_train_colsum: 64-row blocks capped at 64 (then ragged blocks of ceil(rows / 64)), partials added in order, row stride ld > cols, accumulate
    into out.  Integer-valued rows: exact; random rows: fp32 rounding of the per-block sums."""
    from ullsam_amd.training import _row_blocks
    cols, ld = 300, 317
    g = _gen(rows)
    for integer in (True, False):
        x = (_ints((rows, ld), g) if integer else _randn((rows, ld), g)).contiguous()
        out0 = _ints((cols,), g)
        out = out0.clone()
        nb = _row_blocks(rows)
        part = torch.full((nb * cols,), float("nan"), device=DEV) if nb > 1 else None
        _lib().call("ullsam_train_colsum", x.data_ptr(), out.data_ptr(), rows, cols, ld, _p(part), _s())
        ref = out0.double() + x[:, :cols].double().sum(0)
        if integer:
            assert torch.equal(out.double(), ref)
        else:
            _close(out, ref, -(-rows // nb), f"colsum rows={rows}")


def _seg_ref(x, t, smooth):
    """calc_instance_loss with BCEWithLogits (mean over pixels) + Dice per instance, mean over instances (train_joint_v2.py:605-661, 774-812)."""
    bce = F.binary_cross_entropy_with_logits(x, t, reduction="none").mean(-1)
    p = x.sigmoid()
    dice = 1 - (2 * (p * t).sum(-1) + smooth) / (p.sum(-1) + t.sum(-1) + smooth)
    return (bce + dice).mean(), bce.mean(), dice.mean()


@pytest.mark.parametrize("P,npix", [(1, 4096), (3, 4096), (1, 5000), (3, 70001)])
def test_seg_loss_and_backward_against_float64_autograd(P, npix):
    """ullsam_train_seg_loss / _seg_loss_bwd: the three losses and dx (scaled by the incoming gradient) against float64 autograd, logits up to +-40,
    npix a multiple of 1024 or not, the last instance with an empty target mask."""
    g = _gen(P * npix)
    x = (torch.rand((P, npix), device=DEV, generator=g) * 80 - 40).contiguous()
    t = (torch.rand((P, npix), device=DEV, generator=g) < 0.3).float()
    t[-1] = 0.0
    smooth = 1e-7
    sums = torch.zeros((P, 4), device=DEV)
    losses = torch.empty((3,), device=DEV)
    part = torch.full((P * 4 * -(-npix // 1024),), float("nan"), device=DEV)
    _lib().call("ullsam_train_seg_loss", x.data_ptr(), t.data_ptr(), sums.data_ptr(), losses.data_ptr(), P, npix, smooth, part.data_ptr(), _s())
    gs = torch.tensor([0.7], device=DEV)
    dx = torch.empty_like(x)
    _lib().call("ullsam_train_seg_loss_bwd", x.data_ptr(), t.data_ptr(), sums.data_ptr(), gs.data_ptr(), dx.data_ptr(), P, npix, smooth, _s())
    xd = x.double().requires_grad_(True)
    tot, bce, dice = _seg_ref(xd, t.double(), smooth)
    (0.7 * tot).backward()
    for a, r in zip(losses.tolist(), (tot, bce, dice)):
        assert abs(a - float(r)) <= _tol(npix) * max(abs(float(r)), 1e-6), (P, npix, a, float(r))
    _close(dx, xd.grad, npix, "seg_loss dx")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. LayerNorm and RMSNorm backward branches
# ---------------------------------------------------------------------------------------------------------------------------------------------

def _ln_call(x, w, dy, D, rows, eps, params):
    from ullsam_amd.training import _row_blocks
    dx = torch.full_like(x, float("nan"))
    dw = torch.zeros((D,), device=DEV) if params else None
    db = torch.zeros((D,), device=DEV) if params else None
    ws = torch.empty((2 * rows + 2 * _row_blocks(rows) * D,), device=DEV) if params else None
    _lib().call("ullsam_train_ln_bwd", x.data_ptr(), _p(w), dy.data_ptr(), dx.data_ptr(), _p(dw), _p(db), rows, D, eps, _p(ws), _s())
    return dx, dw, db


@pytest.mark.parametrize("D", [4, 6, 96, 512, 516, 1280, 2048, 2052])
@pytest.mark.parametrize("affine", [True, False])
def test_layernorm_backward_branches_against_float64_autograd(D, affine):
    """ullsam_train_ln_bwd: the register kernel with 2 float4 per lane (D <= 512), with 8 (D <= 2048), the per-element kernel (D % 4 != 0, D > 2048,
    misaligned base); rows not a multiple of 4; dw / db from the ordered row-block partials (rows > 64 x 64 for ragged blocks)."""
    rows = 4133 if D in (96, 1280) else 37
    g = _gen(D * 10 + affine)
    x = _randn((rows, D), g, 2.0) + 0.5
    dy = _randn((rows, D), g)
    w = (1 + 0.3 * _randn((D,), g)) if affine else None
    b = (0.1 * _randn((D,), g)) if affine else None
    eps = 1e-6
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True) if affine else None
    bd = b.double().requires_grad_(True) if affine else None
    F.layer_norm(xd, (D,), wd, bd, eps).backward(dy.double())
    variants = [(x, dy, w)]
    if D == 512:
        variants.append((_misaligned(x), _misaligned(dy), w))      # 4 bytes off: the per-element kernel
    for xx, gg, ww in variants:
        dx, dw, db = _ln_call(xx, ww, gg, D, rows, eps, affine)
        _close(dx, xd.grad, D, f"ln dx D={D}")
        if affine:
            _close(dw, wd.grad, rows, f"ln dw D={D}")
            _close(db, bd.grad, rows, f"ln db D={D}")
    if affine:   # dw / db NULL: dx alone, no workspace
        dx, _, _ = _ln_call(x, w, dy, D, rows, eps, False)
        _close(dx, xd.grad, D, f"ln dx (no params) D={D}")


@pytest.mark.parametrize("D,rows,misalign", [(4100, 37, False), (4096, 21, True), (96, 9, True)])
def test_rmsnorm_backward_scalar_kernel_against_float64_autograd(D, rows, misalign):
    """ullsam_train_rmsnorm_bwd on rmsnorm_bwd_kernel (one wave per row): D > 4096 or a base pointer off 16 bytes; with dw_rows and with dw_rows NULL."""
    g = _gen(D + rows)
    x, dy = _randn((rows, D), g), _randn((rows, D), g)
    w = 1 + 0.2 * _randn((D,), g)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    (xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-6) * wd).backward(dy.double())
    if misalign:
        x, dy = _misaligned(x), _misaligned(dy)
    for with_rows in (True, False):
        dx = torch.full((rows, D), float("nan"), device=DEV)
        dw_rows = torch.full((rows, D), float("nan"), device=DEV) if with_rows else None
        _lib().call("ullsam_train_rmsnorm_bwd", x.data_ptr(), w.data_ptr(), dy.data_ptr(), dx.data_ptr(), _p(dw_rows), rows, D, 1e-6, _s())
        _close(dx, xd.grad, D, "rmsnorm dx")
        if with_rows:
            _close(dw_rows.sum(0), wd.grad, rows, "rmsnorm dw")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. adjoint and index kernels
# ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [3, 1023, 1024, 1025, 5000])
@pytest.mark.parametrize("C", [1, 80, 256])
def test_index_add_rows_against_float64(rows, C):
    """ullsam_train_index_add_rows: dst[idx[r]] += src[r] through 1024-entry LDS chunks of the index list, sixteen lanes per element; heavily repeated
    indices (most rows hit three destinations), destination tables of 5 and 127 rows.  Integer-valued src: exact."""
    g = _gen(rows * 7 + C)
    for nd in (5, 127):
        idx = torch.where(torch.rand((rows,), device=DEV, generator=g) < 0.8, torch.randint(0, 3, (rows,), device=DEV, generator=g),
                          torch.randint(0, nd, (rows,), device=DEV, generator=g)).to(torch.int32).contiguous()
        for integer in (True, False):
            src = _ints((rows, C), g) if integer else _randn((rows, C), g)
            dst0 = _ints((nd, C), g)
            dst = dst0.clone()
            _lib().call("ullsam_train_index_add_rows", src.data_ptr(), idx.data_ptr(), dst.data_ptr(), rows, C, nd, _s())
            ref = dst0.double().index_add_(0, idx.long(), src.double())
            if integer:
                assert torch.equal(dst.double(), ref), (rows, C, nd)
            else:
                _close(dst, ref, rows, f"index_add rows={rows} C={C} nd={nd}")


def _im2col64(x):
    """[B, H, W, C] -> [B*H*W, 9*C]: column (ty*3 + tx)*C + c of pixel (y, x) = x[y + ty - 1, x + tx - 1, c], zero outside (image_encoder.py:96-102 as im2col)."""
    B, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    return torch.stack([xp[:, ty:ty + H, tx:tx + W, :] for ty in range(3) for tx in range(3)], 3).reshape(B * H * W, 9 * C)


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 1), (2, 5, 7, 3), (1, 1, 9, 4), (1, 14, 14, 256), (1, 64, 64, 1)])
def test_col2im3x3_is_the_adjoint_of_im2col3x3(B, H, W, C):
    """ullsam_train_col2im3x3 against the float64 gather (autograd of the im2col definition), exactly on integer-valued input, and
    <im2col(x), d> = <x, col2im(d)> (with ullsam_im2col3x3 where C allows it)."""
    from ullsam_amd import ops
    g = _gen(B * H * W * C)
    d = _ints((B * H * W, 9 * C), g)
    dx = torch.full((B * H * W, C), float("nan"), device=DEV)
    _lib().call("ullsam_train_col2im3x3", d.data_ptr(), dx.data_ptr(), B, H, W, C, _s())
    x64 = torch.zeros((B, H, W, C), dtype=torch.float64, device=DEV, requires_grad=True)
    _im2col64(x64).backward(d.double())
    assert torch.equal(dx.double(), x64.grad.reshape(B * H * W, C))
    x = _randn((B * H * W, C), g)
    if C % 4 == 0:                                     # (ullsam_im2col3x3 takes rows of 16-byte multiples)
        cols = ops.im2col3x3(x, B, H, W, C)
        assert torch.equal(cols.double(), _im2col64(x.double().reshape(B, H, W, C)))
    else:
        cols = _im2col64(x.reshape(B, H, W, C))
    dr = _randn((B * H * W, 9 * C), g)
    _lib().call("ullsam_train_col2im3x3", dr.data_ptr(), dx.data_ptr(), B, H, W, C, _s())
    lhs, rhs = float((cols.double() * dr.double()).sum()), float((x.double() * dx.double()).sum())
    assert abs(lhs - rhs) <= 1e-6 * float((cols.double() * dr.double()).abs().sum()), (lhs, rhs)


@pytest.mark.parametrize("ih,iw,oh,ow", [(256, 256, 1024, 1024), (1024, 1024, 256, 256), (64, 64, 1000, 1000), (7, 7, 3, 3), (1, 1, 5, 5), (6, 9, 11, 4)])
def test_resize_backward_against_float64_autograd(ih, iw, oh, ow):
    """ullsam_train_resize_bwd (gather form of the bilinear adjoint) against float64 autograd of F.interpolate(bilinear, align_corners=False),
    up- and down-sampling, non-integer ratios, a 1 x 1 source; accumulates into din."""
    planes = 2
    g = _gen(ih * 31 + oh)
    dout = _randn((planes, oh, ow), g)
    din0 = _randn((planes, ih, iw), g)
    din = din0.clone()
    _lib().call("ullsam_train_resize_bwd", dout.data_ptr(), din.data_ptr(), planes, ih, iw, oh, ow, _s())
    x = torch.zeros((planes, 1, ih, iw), dtype=torch.float64, device=DEV, requires_grad=True)
    F.interpolate(x, (oh, ow), mode="bilinear", align_corners=False).backward(dout.double().reshape(planes, 1, oh, ow))
    ref = x.grad.reshape(planes, ih, iw)
    _close(din - din0, ref, max(1, (oh * ow) // (ih * iw)) * 4, f"resize {ih}x{iw}->{oh}x{ow}")


@pytest.mark.parametrize("adjoint", [0, 1])
def test_rope_and_its_adjoint_against_float64(adjoint):
    """ullsam_train_rope: x cos + rotate_half(x) sin (modeling_internlm2.py:233-247) and, adjoint = 1, its transpose against float64 autograd
    (general tables: the two halves of cos / sin differ, so a swapped or sign-flipped term shows); positions outside the table are clamped."""
    tokens, heads, hd, tab = 300, 3, 64, 100
    g = _gen(adjoint + 11)
    cos, sin = _randn((tab, hd), g), _randn((tab, hd), g)
    pos = torch.randint(0, tab, (tokens,), device=DEV, generator=g).to(torch.int32)
    pos[:4] = torch.tensor([-5, -1, tab, tab + 37], dtype=torch.int32)
    x = _randn((tokens, heads * hd), g)
    out = torch.empty_like(x)
    _lib().call("ullsam_train_rope", x.data_ptr(), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), out.data_ptr(), tokens, heads, hd, tab, adjoint, _s())
    pc = pos.long().clamp(0, tab - 1)
    c, s = cos.double()[pc][:, None, :], sin.double()[pc][:, None, :]

    def fwd(t):
        t = t.reshape(tokens, heads, hd)
        rot = torch.cat([-t[..., hd // 2:], t[..., :hd // 2]], -1)
        return (t * c + rot * s).reshape(tokens, heads * hd)
    if adjoint:
        z = torch.zeros((tokens, heads * hd), dtype=torch.float64, device=DEV, requires_grad=True)
        fwd(z).backward(x.double())
        ref = z.grad
    else:
        ref = fwd(x.double())
    _close(out, ref, 2, "rope")
    # the clamp: the out-of-range rows equal the same rows rotated at positions 0 / tab - 1
    pos2 = pos.clone()
    pos2[:4] = torch.tensor([0, 0, tab - 1, tab - 1], dtype=torch.int32)
    out2 = torch.empty_like(x)
    _lib().call("ullsam_train_rope", x.data_ptr(), pos2.data_ptr(), cos.data_ptr(), sin.data_ptr(), out2.data_ptr(), tokens, heads, hd, tab, adjoint, _s())
    assert torch.equal(out, out2)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. matrix products
# ---------------------------------------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _vec(on):
    lib = _lib().load()
    old = lib.ullsam_train_set_matmul_vec(on)
    try:
        yield
    finally:
        lib.ullsam_train_set_matmul_vec(old)


def _heads_operand(rows_fast, O, Hx, R, Kd, g):
    """An operand of ullsam_train_matmul_heads for O outer entries of Hx heads of [R][Kd] matrices, stored either as activation rows
    [O*R, Hx*Kd] (Kd fastest) or head-major transposed [O, Hx, Kd, R] (R fastest); returns (tensor, (o, h, r, k) strides, float64 [O, Hx, R, Kd])."""
    if rows_fast:
        t = _randn((O * R, Hx * Kd), g)
        st = (R * Hx * Kd, Kd, Hx * Kd, 1)
        v = t.double().reshape(O, R, Hx, Kd).permute(0, 2, 1, 3)
    else:
        t = _randn((O, Hx, Kd, R), g)
        st = (Hx * Kd * R, Kd * R, 1, R)
        v = t.double().permute(0, 1, 3, 2)
    return t, st, v


@pytest.mark.parametrize("M,N,K", [(196, 196, 80), (129, 64, 64), (40, 33, 24), (64, 48, 16)])
@pytest.mark.parametrize("hdiv", [1, 4])
def test_matmul_heads_against_float64_einsum(M, N, K, hdiv):
    """ullsam_train_matmul_heads over (outer, head) pairs: all four operand layouts (A k- or m-fastest, B n- or k-fastest), grouped B heads
    (head divisor 4: KV heads), accumulate; fp32 (MFMA and, below 64 x 48 x 16, the scalar kernel) and bf16 with 16-byte and per-element fetches
    (bit-equal), a misaligned base (per-element fetches) against float64 of the bf16-rounded operands."""
    O, Hh = 2, 4
    g = _gen(M * N + K + hdiv)
    for a_rows in (True, False):
        for b_kfast in (True, False):
            A, sa, Av = _heads_operand(a_rows, O, Hh, M, K, g)                   # A [o][h] = [M][K]
            Bt, sbt, Bv = _heads_operand(b_kfast, O, Hh // hdiv, N, K, g)       # stored as [N][K] (k fastest: rows) or [K][N]... as (o, h, n, k)
            sb = (sbt[0], sbt[1], sbt[3], sbt[2])                                 # (o, h, k, n) strides of B = that operand read transposed
            Bref = Bv.repeat_interleave(hdiv, 1).transpose(2, 3)                  # [O, Hh, K, N]
            C0 = _randn((O, Hh, M, N), g)
            ref = torch.einsum("ohmk,ohkn->ohmn", Av, Bref)
            refb = torch.einsum("ohmk,ohkn->ohmn", Av.float().bfloat16().double(), Bref.float().bfloat16().double())
            outs = {}
            for bf16, vec, mis in ((0, 1, False), (1, 1, False), (1, 0, False), (1, 1, True)):
                AA = _misaligned(A) if mis else A
                for acc in (0, 1):
                    C = C0.clone()
                    with _vec(vec):
                        _lib().call("ullsam_train_matmul_heads", AA.data_ptr(), Bt.data_ptr(), C.data_ptr(), M, N, K, O, Hh, sa[0], sa[1], 1, sa[2], sa[3],
                                    sb[0], sb[1], hdiv, sb[2], sb[3], Hh * M * N, M * N, N, 1, acc, bf16, 0, _s())
                    r = refb if (bf16 and M >= 64 and N >= 48 and K >= 16) else ref      # (below the MFMA tile the bf16 product is the fp32 one)
                    _close(C - C0 if acc else C, r, K, f"heads M={M} N={N} K={K} a_rows={a_rows} b_kfast={b_kfast} bf16={bf16} vec={vec} acc={acc}")
                    outs[(bf16, vec, mis, acc)] = C
            assert torch.equal(outs[(1, 1, False, 0)], outs[(1, 0, False, 0)]), "bf16 product: vec on / off not bit-equal"
            assert torch.equal(outs[(1, 1, False, 0)], outs[(1, 1, True, 0)]), "bf16 product: misaligned base not bit-equal"


@pytest.mark.parametrize("S", [64, 129, 255, 256, 1081])
@pytest.mark.parametrize("bf16", [0, 1])
def test_matmul_heads_causal_tiles_equal_the_whole_product(S, bf16):
    """`tri` of ullsam_train_matmul_heads on a square causal attention, heads read in place from [S, H*hd] rows: tri = 1 (C = Q K^T, tiles behind the
    diagonal not formed) equals tri = 0 bit for bit on every formed 128 x 128 tile; tri = 2 (dK = dS^T Q, sums start at the tile's first key) and tri = 3
    (out = P V, sums stop after the tile's last query) equal tri = 0 bit for bit on a causally zeroed P, and float64."""
    O, H, hd = 2, 2, 64
    g = _gen(S * 3 + bf16)
    q, k = _randn((O * S, H * hd), g), _randn((O * S, H * hd), g)
    rows = (S * H * hd, hd, 1, H * hd, 1)
    sC = (H * S * S, S * S, S, 1)

    def run(A, sa, Bm, sb, M, N, K, sc, tri, Cshape):
        C = torch.full(Cshape, float("nan"), device=DEV) if tri == 1 else torch.zeros(Cshape, device=DEV)
        _lib().call("ullsam_train_matmul_heads", A.data_ptr(), Bm.data_ptr(), C.data_ptr(), M, N, K, O, H, sa[0], sa[1], sa[2], sa[3], sa[4],
                    sb[0], sb[1], sb[2], sb[3], sb[4], sc[0], sc[1], sc[2], sc[3], 0, bf16, tri, _s())
        return C
    rd = lambda t: (t.bfloat16() if bf16 else t).double()
    kT = (S * H * hd, hd, 1, 1, H * hd)
    full = run(q, rows, k, kT, S, S, hd, sC, 0, (O, H, S, S))
    clip = run(q, rows, k, kT, S, S, hd, sC, 1, (O, H, S, S))
    i = torch.arange(S, device=DEV)
    formed = (i[None, :] // 128) <= (i[:, None] // 128)
    assert torch.equal(full[..., formed], clip[..., formed])
    qh = rd(q).reshape(O, S, H, hd).permute(0, 2, 1, 3)
    kh = rd(k).reshape(O, S, H, hd).permute(0, 2, 1, 3)
    _close(full, qh @ kh.transpose(2, 3), hd, "Q K^T")
    causal = (i[None, :] <= i[:, None]).float()
    P = (_randn((O, H, S, S), g).abs() * causal).contiguous()
    v = _randn((O * S, H * hd), g)
    vh = rd(v).reshape(O, S, H, hd).permute(0, 2, 1, 3)
    rowsC = (S * H * hd, hd, H * hd, 1)
    sP, sPT = (H * S * S, S * S, 1, S, 1), (H * S * S, S * S, 1, 1, S)
    o0 = run(P, sP, v, rows, S, hd, S, rowsC, 0, (O * S, H * hd))
    o3 = run(P, sP, v, rows, S, hd, S, rowsC, 3, (O * S, H * hd))
    assert torch.equal(o0, o3)
    _close(o0.reshape(O, S, H, hd).permute(0, 2, 1, 3), rd(P) @ vh, S, "P V")
    d0 = run(P, sPT, q, rows, S, hd, S, rowsC, 0, (O * S, H * hd))
    d2 = run(P, sPT, q, rows, S, hd, S, rowsC, 2, (O * S, H * hd))
    assert torch.equal(d0, d2)
    _close(d0.reshape(O, S, H, hd).permute(0, 2, 1, 3), rd(P).transpose(2, 3) @ qh, S, "P^T Q")


@pytest.mark.parametrize("M,N,K,batch,ksplit", [(14, 80, 1000, 3, 7), (64, 48, 4100, 2, 5), (5, 32, 100, 2, 4), (70, 50, 65, 1, 3), (14, 80, 5600, 14, 43)])
def test_matmul_splitk_against_float64(M, N, K, batch, ksplit):
    """ullsam_train_matmul_splitk called directly: k pieces of ceil(K / ksplit) rounded up to 32, a short last piece (down to one term), fewer pieces than
    asked when the rounding covers K early; partials added in order; accumulate.  Against float64 and the one-launch product."""
    g = _gen(M * K + ksplit)
    A = _randn((batch, K, M), g)                # read transposed (m fastest), as the table gradients do
    Bm = _randn((batch, K, N), g)
    C0 = _randn((batch, M, N), g)
    ref = A.double().transpose(1, 2) @ Bm.double()
    for acc in (0, 1):
        C = C0.clone()
        part = torch.full((ksplit * batch * M * N,), float("nan"), device=DEV)
        _lib().call("ullsam_train_matmul_splitk", A.data_ptr(), Bm.data_ptr(), C.data_ptr(), M, N, K, batch, K * M, 1, M, K * N, N, 1, M * N, N, 1, acc,
                    ksplit, part.data_ptr(), _s())
        _close(C - C0 if acc else C, ref, K, f"splitk acc={acc}")
    one = torch.empty_like(C0)
    _lib().call("ullsam_train_matmul", A.data_ptr(), Bm.data_ptr(), one.data_ptr(), M, N, K, batch, K * M, 1, M, K * N, N, 1, M * N, N, 1, 0, _s())
    _close(one, ref, K, "one-launch")


@pytest.mark.parametrize("M,N,K,a_t", [(196, 80, 196, False), (64, 48, 16, True), (257, 129, 1081, True), (40, 60, 33, False)])
def test_matmul_bf16_against_float64_of_rounded_operands(M, N, K, a_t):
    """ullsam_train_matmul_bf16 called directly (batched, A row-major or read transposed): float64 of the bf16-rounded operands on the MFMA path, the
    fp32 product below its tile; 16-byte and per-element fetches and a misaligned base give the same bits."""
    batch = 3
    g = _gen(M + N * 3 + K)
    A = _randn((batch, K, M) if a_t else (batch, M, K), g)
    Bm = _randn((batch, K, N), g)
    sa = (M * K, 1, M) if a_t else (M * K, K, 1)
    mfma = M >= 64 and N >= 48 and K >= 16
    rd = (lambda t: t.bfloat16().double()) if mfma else (lambda t: t.double())
    ref = (rd(A).transpose(1, 2) if a_t else rd(A)) @ rd(Bm)
    outs = []
    for vec, mis in ((1, False), (0, False), (1, True)):
        AA = _misaligned(A) if mis else A
        C = torch.full((batch, M, N), float("nan"), device=DEV)
        with _vec(vec):
            _lib().call("ullsam_train_matmul_bf16", AA.data_ptr(), Bm.data_ptr(), C.data_ptr(), M, N, K, batch, *sa, K * N, N, 1, M * N, N, 1, 0, _s())
        _close(C, ref, K, f"matmul_bf16 vec={vec} misaligned={mis}")
        outs.append(C)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_per_query_attention_kernel_with_strided_operands_against_float64():
    """ullsam_train_attention (one workgroup per query; the backward adds dk / dv by atomics) called directly on operands with (batch, token, head)
    strides that are not those of contiguous rows: q / out token-major inside a wider buffer, k / v head-major, grouped KV heads, causal offset and
    a key mask; forward out and backward dq / dk / dv against float64 autograd."""
    B, H, KVH, hd, Sq, Sk, causal = 2, 4, 2, 32, 9, 40, 31
    G = H // KVH
    g = _gen(77)
    qbuf = _randn((B, Sq, H * hd + 16), g)                                  # token stride H*hd + 16
    kb, vb = _randn((B, KVH, Sk, hd), g), _randn((B, KVH, Sk, hd), g)        # head-major
    dob = _randn((B, Sq, H * hd + 16), g)
    km = torch.ones((B, Sk), dtype=torch.int32, device=DEV)
    km[0, :12] = 0
    km[1, 30:] = 0
    qs = (Sq * (H * hd + 16), H * hd + 16, hd)
    ks = (KVH * Sk * hd, hd, Sk * hd)
    out = torch.zeros_like(qbuf)
    dq = torch.zeros_like(qbuf)
    dk, dv = torch.zeros_like(kb), torch.zeros_like(vb)
    sc = 1.0 / math.sqrt(hd)
    for dout, o, dqq in ((None, out, None), (dob, None, dq)):
        _lib().call("ullsam_train_attention", qbuf.data_ptr(), kb.data_ptr(), vb.data_ptr(), _p(dout), _p(o), _p(dqq), _p(dk if dout is not None else None),
                    _p(dv if dout is not None else None), B, H, G, hd, Sq, Sk, causal, km.data_ptr(), *qs, *ks, *ks, *qs, sc, None, None, None, None, 0, _s())
    qd = qbuf.double()[..., :H * hd].reshape(B, Sq, H, hd).permute(0, 2, 1, 3).detach().requires_grad_(True)
    kd, vd = kb.double().requires_grad_(True), vb.double().requires_grad_(True)
    s = qd @ kd.repeat_interleave(G, 1).transpose(2, 3) * sc
    p = torch.softmax(_masked_logits(s, _ref_mask(B, Sq, Sk, causal, km)), -1)
    o_ref = p @ vd.repeat_interleave(G, 1)
    o_ref.backward(dob.double()[..., :H * hd].reshape(B, Sq, H, hd).permute(0, 2, 1, 3))
    _close(out[..., :H * hd].reshape(B, Sq, H, hd).permute(0, 2, 1, 3), o_ref.detach(), Sk, "out")
    _close(dq[..., :H * hd].reshape(B, Sq, H, hd).permute(0, 2, 1, 3), qd.grad, Sk, "dq")
    _close(dk, kd.grad, Sq * G, "dk")
    _close(dv, vd.grad, Sq * G, "dv")
    assert float(out[..., H * hd:].abs().max()) == 0.0 and float(dq[..., H * hd:].abs().max()) == 0.0     # nothing written between the rows


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. the attention row pass against its definition
# ---------------------------------------------------------------------------------------------------------------------------------------------

def _ref_mask(B, Sq, Sk, causal, km):
    """The reference's additive mask in fp32 [B, 1, Sq, Sk]: _make_causal_mask (finfo.min where key > query + past) + _expand_mask (finfo.min on padded
    keys), summed in fp32 (a doubly masked entry is -inf) -- modeling_internlm2.py:96-125, 830-851."""
    m = torch.zeros((B, 1, Sq, Sk), device=DEV)
    if causal >= 0:
        i, j = torch.arange(Sq, device=DEV)[:, None], torch.arange(Sk, device=DEV)[None, :]
        m = m + torch.where(j > i + causal, torch.tensor(FMIN, device=DEV), torch.tensor(0.0, device=DEV))
    if km is not None:
        inv = 1.0 - km.float()[:, None, None, :].expand(B, 1, Sq, Sk)
        m = inv.masked_fill(inv.bool(), FMIN) + m
    return m


def _masked_logits(s, m):
    """s + m as fp32 evaluates it (a masked entry is finfo.min or -inf whatever the score), with the gradient of s + m (1 everywhere), in float64."""
    m = m.double()
    return s + torch.where(m == 0, torch.zeros_like(m), m - s).detach()


def _key_mask(kind, B, Sk):
    km = torch.ones((B, Sk), dtype=torch.int32, device=DEV)
    if kind == "right":
        km[0, Sk - 20:] = 0
    elif kind == "left":
        km[0, :37] = 0
        if B > 1:
            km[1, :3] = 0
    elif kind == "mixed":                                  # left padding, a fully padded entry, an unpadded one
        km[0, :Sk // 3] = 0
        km[1, :] = 0
    return None if kind == "none" else km


@pytest.mark.parametrize("Sq,Sk,kw,causal", [(196, 196, 14, 0), (50, 196, 14, 146), (300, 1000, 100, -1), (120, 1000, 0, 880), (64, 2000, 100, 0),
                                             (40, 4096, 64, 4056), (30, 4200, 100, -1), (20, 4200, 0, 0)])
def test_attention_row_pass_against_float64_softmax(Sq, Sk, kw, causal):
    """ullsam_train_attn_rows in all five forms (register kernel for Sk <= 256 / 1024 / 2048 / 4096, the three-pass kernel above) against float64 softmax
    of S + decomposed bias + the reference's masks: causal offsets, left padding of different lengths, a fully padded batch entry, rows whose visible
    keys are all padded (uniform over every single-masked entry); dS and the bias-gradient rows against float64 autograd; have_p 0 and 1."""
    B, H = 3, 2
    g = _gen(Sq * 7 + Sk + causal)
    S0 = _randn((B * H, Sq, Sk), g, 3.0)
    dP0 = _randn((B * H, Sq, Sk), g)
    bh = bw = None
    if kw:
        bh, bw = _randn((B * H, Sq, Sk // kw), g), _randn((B * H, Sq, kw), g)
    km = _key_mask("mixed", B, Sk)
    # float64 definition
    Sd = S0.double().requires_grad_(True)
    lg = Sd.reshape(B, H, Sq, Sk)
    bhd = bwd = None
    if kw:
        bhd, bwd = bh.double().requires_grad_(True), bw.double().requires_grad_(True)
        lg = lg + (bhd.repeat_interleave(kw, -1) + bwd.repeat(1, 1, Sk // kw)).reshape(B, H, Sq, Sk)
    Pd = torch.softmax(_masked_logits(lg, _ref_mask(B, Sq, Sk, causal, km)), -1)
    (Pd * dP0.double().reshape(B, H, Sq, Sk)).sum().backward()
    Pref = Pd.detach().reshape(B * H, Sq, Sk)
    for have_p in (0, 1):
        P = S0.clone()
        dS = dP0.clone()
        dbh = torch.full_like(bh, float("nan")) if kw else None
        dbw = torch.full_like(bw, float("nan")) if kw else None
        if have_p:
            _lib().call("ullsam_train_attn_rows", P.data_ptr(), None, _p(bh), _p(bw), None, None, _p(km), B, H, Sq, Sk, max(kw, 1), causal, 0, _s())
            assert float((P.double() - Pref).abs().max()) <= 1e-5, float((P.double() - Pref).abs().max())
        _lib().call("ullsam_train_attn_rows", P.data_ptr(), dS.data_ptr(), _p(bh), _p(bw), _p(dbh), _p(dbw), _p(km), B, H, Sq, Sk, max(kw, 1), causal, have_p, _s())
        assert float((P.double() - Pref).abs().max()) <= 1e-5, (have_p, float((P.double() - Pref).abs().max()))
        # (P carries the rounding of logits up to ~15 in size through expf: a few 1e-6 of P; dS and the bias rows are held to 1e-5 of their scale)
        _close(dS, Sd.grad, 1 << 20, f"dS have_p={have_p}")
        if kw:
            _close(dbh, bhd.grad, 1 << 20, "dbias_h")
            _close(dbw, bwd.grad, 1 << 20, "dbias_w")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. AttentionFn route by route against float64 autograd; 7. the switches documented as giving the same bits
# ---------------------------------------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _switches(**kw):
    from ullsam_amd import training as T
    old = {k: getattr(T, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(T, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(T, k, v)


def _attn_ref(q, k, v, B, H, KVH, Sq, Sk, causal, km, bh, bw, kw, dout, autocast=False):
    """The reference's attention (modeling_internlm2.py:383-419 / image_encoder.py:224-240) and its autograd: float64, or fp32 under autocast(bfloat16)."""
    hd = q.shape[1] // H
    G = H // KVH
    cast = (lambda t: t.float()) if autocast else (lambda t: t.double())
    leaves = [cast(t).detach().requires_grad_(True) for t in (q, k, v)]
    lb = [cast(t).detach().requires_grad_(True) for t in (bh, bw)] if bh is not None else []
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if autocast else contextlib.nullcontext()
    with ctx:
        qh = leaves[0].reshape(B, Sq, H, hd).transpose(1, 2)
        kh = leaves[1].reshape(B, Sk, KVH, hd).transpose(1, 2).repeat_interleave(G, 1)
        vh = leaves[2].reshape(B, Sk, KVH, hd).transpose(1, 2).repeat_interleave(G, 1)
        s = torch.matmul(qh, kh.transpose(2, 3)) / math.sqrt(hd)
        if lb:
            s = s + (lb[0].repeat_interleave(kw, -1) + lb[1].repeat(1, 1, 1, Sk // kw))
        m = _ref_mask(B, Sq, Sk, causal, km) if (causal >= 0 or km is not None) else None
        if m is not None:
            s = (s.float() + m) if autocast else _masked_logits(s, m)
        p = torch.softmax(s, -1, dtype=torch.float32 if autocast else torch.float64)
        if autocast:
            p = p.to(torch.bfloat16)
        out = torch.matmul(p, vh).transpose(1, 2).reshape(B * Sq, H * hd)
    out.backward(cast(dout))
    return [out.detach().double()] + [t.grad.double() for t in leaves + lb]


def _attn_run(q, k, v, B, H, KVH, Sq, Sk, causal, km, bh, bw, kw, dout, bf16=False):
    from ullsam_amd.training import AttentionFn
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    lb = [t.clone().requires_grad_(True) for t in (bh, bw)] if bh is not None else []
    out = AttentionFn.apply(*leaves, B, H, KVH, Sq, Sk, causal, km, lb[0] if lb else None, lb[1] if lb else None, kw, bf16)
    out.backward(dout)
    torch.cuda.synchronize()
    return [out.detach()] + [t.grad for t in leaves + lb]


_NAMES = ("out", "dq", "dk", "dv", "dbias_h", "dbias_w")
_FP32_ROUTES = {
    "inplace": dict(),
    "tri_off": dict(TRI_CAUSAL=False),
    "keep_p": dict(RECOMPUTE_P=False),
    "head_major": dict(INPLACE_ATTN=False),
    "per_query": dict(MATRIX_ATTN_FROM=1 << 62),
}
_CASES = ([("decoder_cross", 1, 8, 8, 7, 4096, 16, -1, "none", 0), ("vit_window", 3, 2, 2, 196, 196, 80, -1, "none", 14),
           ("vit_global", 1, 2, 2, 1024, 1024, 80, -1, "none", 32)]
          + [(f"llm_hd{hd}_S{S}_{mk}", 2, 8, 2, S, S, hd, 0, mk, 0) for hd in (64, 128) for S in (129, 300, 1081) for mk in ("none", "right", "left")])


def _attn_inputs(B, H, KVH, Sq, Sk, hd, mk, kw, seed):
    g = _gen(seed)
    q, k, v = _randn((B * Sq, H * hd), g), _randn((B * Sk, KVH * hd), g), _randn((B * Sk, KVH * hd), g)
    dout = _randn((B * Sq, H * hd), g)                       # nonzero on every row, padded rows included
    bh = bw = None
    if kw:
        bh, bw = _randn((B, H, Sq, Sk // kw), g), _randn((B, H, Sq, kw), g)
    return q, k, v, dout, _key_mask(mk, B, Sk), bh, bw


@pytest.mark.parametrize("case", _CASES, ids=[c[0] for c in _CASES])
def test_attention_fn_fp32_routes_against_float64_autograd(case):
    """AttentionFn in fp32 by route (in place on the row tensors with causal tile clipping, TRI_CAUSAL off, the forward's P kept (RECOMPUTE_P off),
    head-major copies, the per-query kernel): out, dq, dk, dv (and the decomposed-bias gradients) against float64 autograd of the reference's attention
    with a random dO on every row, left-padded rows included.  TRI_CAUSAL and RECOMPUTE_P are documented as giving the same bits: asserted exactly."""
    name, B, H, KVH, Sq, Sk, hd, causal, mk, kw = case
    q, k, v, dout, km, bh, bw = _attn_inputs(B, H, KVH, Sq, Sk, hd, mk, kw, zlib.crc32(name.encode()))
    ref = _attn_ref(q, k, v, B, H, KVH, Sq, Sk, causal, km, bh, bw, kw, dout)
    res = {}
    for route, sw in _FP32_ROUTES.items():
        with _switches(**sw):
            res[route] = _attn_run(q, k, v, B, H, KVH, Sq, Sk, causal, km, bh, bw, kw, dout)
        n_sum = (Sk, Sk, Sq, Sq, kw, Sk // max(kw, 1))
        for nm, a, r, n in zip(_NAMES, res[route], ref, n_sum):
            _close(a, r, max(n, hd), f"{name} {route} {nm}")
    for route in ("tri_off", "keep_p"):
        for nm, a, b in zip(_NAMES, res["inplace"], res[route]):
            assert torch.equal(a, b), f"{name}: {route} is not bit-equal to the default route ({nm})"


_BF16_CASES = ([("vit_window", 3, 2, 2, 196, 196, 80, -1, "none", 14), ("vit_global", 1, 2, 2, 1024, 1024, 80, -1, "none", 32)]
               + [(f"llm_hd128_S{S}_{mk}", 2, 8, 2, S, S, 128, 0, mk, 0) for S in (129, 1081) for mk in ("none", "right", "left")])


@pytest.mark.parametrize("case", _BF16_CASES, ids=[c[0] for c in _BF16_CASES])
def test_attention_fn_bf16_routes_within_the_autocast_error(case):
    """AttentionFn with bf16 products (a bf16 model's attention: operands rounded to bf16, fp32 accumulation and softmax) by route -- the LLM forward
    on the inference path's causal kernel (FUSED_CAUSAL_FWD), the matrix form in place, head-major -- against float64: every tensor within 1.5x the
    error of torch's own autocast(bfloat16) on the reference's code plus a floor of 1e-3 of the scale."""
    name, B, H, KVH, Sq, Sk, hd, causal, mk, kw = case
    q, k, v, dout, km, bh, bw = _attn_inputs(B, H, KVH, Sq, Sk, hd, mk, kw, zlib.crc32(name.encode()) + 1)
    ref = _attn_ref(q, k, v, B, H, KVH, Sq, Sk, causal, km, bh, bw, kw, dout)
    auto = _attn_ref(q, k, v, B, H, KVH, Sq, Sk, causal, km, bh, bw, kw, dout, autocast=True)
    for route, sw in {"fused_fwd": dict(), "matrix_fwd": dict(FUSED_CAUSAL_FWD=False), "head_major": dict(INPLACE_ATTN=False)}.items():
        with _switches(**sw):
            got = _attn_run(q, k, v, B, H, KVH, Sq, Sk, causal, km, bh, bw, kw, dout, bf16=True)
        for nm, a, r, t in zip(_NAMES, got, ref, auto):
            e, et, sc = _err(a, r), _err(t, r), _scale(r)
            assert torch.isfinite(a).all() and e <= 1.5 * et + 1e-3 * sc, f"{name} {route} {nm}: err {e:.3e}, autocast {et:.3e}, scale {sc:.3e}"


def test_left_padded_rows_take_the_whole_matrices():
    """A causal attention whose first rows see only padded keys: the reference's softmax of those rows is uniform over every single-masked entry, the
    keys behind the diagonal included, so the clipped products (TRI_CAUSAL) and the causal forward kernel must not be used there.  AttentionFn reads
    that from the key mask when it is not told, and the LLM slice passes it from the host."""
    from ullsam_amd import training as T
    km = _key_mask("left", 2, 300)
    assert T._masked_rows(km, 0) and not T._masked_rows(_key_mask("right", 2, 300), 0) and not T._masked_rows(None, 0)
    dims = (2, 8, 2, 64, 300, 300, 0, 0)
    assert T._tri(dims, False) and not T._tri(dims, True)
