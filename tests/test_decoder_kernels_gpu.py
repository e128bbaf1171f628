"""The fused mask-decoder kernels -- ullsam_dec_tok_attn, ullsam_dec_tok_mlp, ullsam_dec_heads (csrc/dectok.hip), ullsam_i2t_block, ullsam_kv_proj,
ullsam_up1_ln_gelu, ullsam_up2_hyper_masks (csrc/decoder.hip) -- one launch at a time through their C entry points, against the float64 definitions of
tests/decoder_ref.py (written from the reference, checked against the numpy oracle in tests/test_decoder_ref_cpu.py), at the smallest shapes where their
paths divide: every token count around the tile boundaries, null biases / LayerNorm parameters, mode 1 and do_mlp 0, partial row groups, idle waves,
multi-trip loops with ragged ends, non-square grids; every output buffer carries sentinel rows behind its end.

Limits.  The two-term kernels (dec_tok_attn, dec_tok_mlp, dec_heads) declare two bf16 terms per activation, ~8 bits more than one term: per output tensor
max |got - D| <= max |D1 - D| / 64 and rms(got - D) <= rms(D1 - D) / 64, with D1 the ONE-term evaluation of the definition on the same inputs (the yardstick
comes from the definitions alone; the declared arithmetic D2 sits ~10x inside, test_decoder_ref_cpu.py).  i2t_block: rms <= rms(D1 - D) / 8 (D2 sits 4 - 5x
inside) and every element inside decoder_ref.i2t_bound (one bf16 step of EVERY element of its declared bf16-cast attention output at once, fp32 terms, through
the LayerNorm's derivative: 3 - 10x above D1's largest error, so this check catches gross local errors only; the rms limit and the exact-selection inputs
are the sharp ones);
exact-selection inputs have no such steps and get the fp32 terms alone.  bf16 outputs: one bf16 rounding of the float64 value (+ the fp32 terms), elementwise.
Measured err / limit ratios are recorded in each docstring (MI355X)."""
import itertools

import pytest
import torch

from tests import decoder_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7777.0
GUARD = 3            # sentinel rows behind every output


@pytest.fixture(scope="module")
def ops():
    from ullsam_amd import ops as o
    return o


def _call(name, *args):
    from ullsam_amd import _lib as L
    L.call(name, *args, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _p(t):
    return None if t is None else t.data_ptr()


def _within(got, ref64, bound, what):
    """|got - ref| <= bound elementwise (bound: scalar or tensor), everything finite; prints the worst error and the worst share of its bound."""
    got64 = got.double()
    assert got64.shape == ref64.shape, (what, got64.shape, ref64.shape)
    assert bool(torch.isfinite(got64).all()), f"{what}: non-finite values"
    e = (got64 - ref64).abs()
    b = bound if torch.is_tensor(bound) else torch.full_like(e, float(bound))
    ratio = float((e / b.clamp(min=1e-300)).max()) if e.numel() else 0.0
    print(f"{what}: max |err| {float(e.max()) if e.numel() else 0.0:.3e}, worst err / bound {ratio:.3f}")
    assert bool((e <= b).all()), f"{what}: max |err| {float(e.max()):.3e}, worst err / bound {ratio:.3f}"
    return ratio


def _out(rows, cols, dtype=torch.float32):
    """an output buffer of rows + GUARD rows, all sentinel"""
    return torch.full((rows + GUARD, cols), SENT, dtype=dtype, device=DEV)


def _guard_kept(buf, rows, what):
    assert bool((buf[rows:] == torch.tensor(SENT, dtype=buf.dtype)).all()), f"{what}: rows behind the output were written"
    assert not bool((buf[:rows] == torch.tensor(SENT, dtype=buf.dtype)).any()), f"{what}: output rows left unwritten"


def _two_term(outs, what):
    """outs: [(name, got, D, D1)]: max and rms of got - D within 1/64 of the one-term definition's; -> the worst err / limit"""
    worst = 0.0
    for name, got, D, D1 in outs:
        assert got.shape == D.shape and bool(torch.isfinite(got).all()), (what, name)
        (em, er), (lm, lr) = R.err(got, D), R.err(D1, D)
        assert lm > 0 and lr > 0, (what, name)
        print(f"{what} {name}: max |err| {em:.2e} (limit {lm / 64:.2e}: {em / (lm / 64):.3f}), rms {er:.2e} (limit {lr / 64:.2e}: {er / (lr / 64):.3f})")
        assert em <= lm / 64 and er <= lr / 64, (what, name, em, lm / 64, er, lr / 64)
        worst = max(worst, em / (lm / 64), er / (lr / 64))
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------------------
# dec_tok_attn
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _run_tok_attn(ops, d, skip_pe, mode, bufs=None):
    """d: a decoder_ref.tok_attn_case on the device (None entries = NULL operands) -> (queries_out, q_t2i) buffers with guard rows"""
    P, T, _ = d["queries"].shape
    qo, q2 = bufs if bufs is not None else (_out(P * T, 256), _out(P * T, 128))
    pk = {n: (None if d[n] is None else ops.pack_mfma_rows(d[n])) for n in ("Wq", "Wk", "Wv", "Wo", "Wq2")}
    _call("ullsam_dec_tok_attn", d["queries"].data_ptr(), d["qpe"].data_ptr(), _p(qo), q2.data_ptr(), _p(pk["Wq"]), _p(d["bq"]), _p(pk["Wk"]), _p(d["bk"]), _p(pk["Wv"]),
          _p(d["bv"]), _p(pk["Wo"]), _p(d["bo"]), _p(d["ln_w"]), _p(d["ln_b"]), float(d["eps"]), pk["Wq2"].data_ptr(), _p(d["bq2"]), P, T, int(skip_pe), int(mode))
    return qo, q2


@pytest.mark.parametrize("P", R.TOK_P)
@pytest.mark.parametrize("T", R.TOK_T)
def test_dec_tok_attn_against_float64(ops, P, T):
    """mode 0 with and without the first layer's rule (skip_pe), and mode 1 with every self-attention operand NULL: there queries_out stays untouched and
    q_t2i is the projection of queries + qpe whatever skip_pe says.  Measured worst err / limit over the twelve (P, T): max 0.126, rms 0.127 (the declared
    two-term arithmetic D2 itself sits at ~0.1: the kernel adds fp32 accumulation to it)."""
    d = R.to(R.tok_attn_case(P, T), DEV)
    worst = 0.0
    for skip_pe in (0, 1):
        qo, q2 = _run_tok_attn(ops, d, skip_pe, 0)
        D, D1 = (R.tok_attn(*R.tok_attn_args(d, skip_pe, 0, r)) for r in (R.ident, R.bf1))
        worst = max(worst, _two_term([("queries", qo[:P * T].reshape(P, T, 256), D[0], D1[0]), ("q_t2i", q2[:P * T].reshape(P, T, 128), D[1], D1[1])],
                                     f"dec_tok_attn P={P} T={T} skip_pe={skip_pe}"))
        _guard_kept(qo, P * T, "queries_out"); _guard_kept(q2, P * T, "q_t2i")
    D, D1 = (R.tok_attn(*R.tok_attn_args(d, 0, 1, r))[1] for r in (R.ident, R.bf1))
    d1 = dict(d, Wq=None, Wk=None, Wv=None, Wo=None, bq=None, bk=None, bv=None, bo=None, ln_w=None, ln_b=None)
    got = []
    for skip_pe in (0, 1):
        qo, q2 = _run_tok_attn(ops, d1, skip_pe, 1)
        assert bool((qo == SENT).all()), "mode 1 wrote queries_out"
        _guard_kept(q2, P * T, "q_t2i (mode 1)")
        got.append(q2)
    assert torch.equal(got[0], got[1])
    worst = max(worst, _two_term([("q_t2i", got[0][:P * T].reshape(P, T, 128), D, D1)], f"dec_tok_attn P={P} T={T} mode=1"))
    print(f"dec_tok_attn P={P} T={T}: worst err / limit {worst:.3f}")


def test_dec_tok_attn_null_biases_and_layernorm_parameters(ops):
    """all five biases and both LayerNorm parameters NULL (weight 1, bias 0).  Measured worst err / limit: max 0.120, rms 0.098."""
    d, skips, _ = R.tok_attn_special("nulls")
    d = R.to(d, DEV)
    P, T, _ = d["queries"].shape
    for skip_pe in skips:
        qo, q2 = _run_tok_attn(ops, d, skip_pe, 0)
        D, D1 = (R.tok_attn(*R.tok_attn_args(d, skip_pe, 0, r)) for r in (R.ident, R.bf1))
        _two_term([("queries", qo[:P * T].reshape(P, T, 256), D[0], D1[0]), ("q_t2i", q2[:P * T].reshape(P, T, 128), D[1], D1[1])], f"dec_tok_attn nulls skip_pe={skip_pe}")


def test_dec_tok_attn_constant_row_before_the_norm(ops):
    """zero out-projection weights, no bias, no residual (skip_pe): the pre-norm rows are zero, their variance is 0, and norm1 gives ln_b EXACTLY (finite:
    rsqrt(eps) times an exact 0); q_t2i is then the projection of ln_b + qpe.  Measured err / limit (q_t2i): max 0.078, rms 0.094."""
    d = R.to(R.tok_attn_special("constant_row")[0], DEV)
    P, T, _ = d["queries"].shape
    qo, q2 = _run_tok_attn(ops, d, 1, 0)
    assert bool(torch.isfinite(qo).all())
    assert torch.equal(qo[:P * T], d["ln_b"][None].expand(P * T, -1))
    D, D1 = (R.tok_attn(*R.tok_attn_args(d, 1, 0, r)) for r in (R.ident, R.bf1))
    assert float((D[0] - d["ln_b"].double()).abs().max()) == 0.0
    _two_term([("q_t2i", q2[:P * T].reshape(P, T, 128), D[1], D1[1])], "dec_tok_attn constant row")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# dec_tok_mlp
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _run_tok_mlp(ops, d, do_mlp):
    P, T, _ = d["queries"].shape
    qo, ko, vo = _out(P * T, 256), _out(P * T, 128), _out(P * T, 128)
    pk = {n: (None if d[n] is None else ops.pack_mfma_rows(d[n])) for n in ("Wo", "W1", "W2", "Wk", "Wv")}
    on = bool(do_mlp)
    _call("ullsam_dec_tok_mlp", d["queries"].data_ptr(), d["attn"].data_ptr(), _p(d["qpe"]) if on else None, qo.data_ptr(), _p(ko) if on else None, _p(vo) if on else None,
          pk["Wo"].data_ptr(), _p(d["bo"]), _p(d["ln2_w"]), _p(d["ln2_b"]), float(d["eps"]), _p(pk["W1"]) if on else None, _p(d["b1"]) if on else None,
          _p(pk["W2"]) if on else None, _p(d["b2"]) if on else None, _p(d["ln3_w"]) if on else None, _p(d["ln3_b"]) if on else None, float(d["eps"]) if on else 0.0,
          _p(pk["Wk"]) if on else None, _p(d["bk"]) if on else None, _p(pk["Wv"]) if on else None, _p(d["bv"]) if on else None, P, T, int(do_mlp))
    return qo, ko, vo


def _check_tok_mlp(ops, d, do_mlp, what):
    P, T, _ = d["queries"].shape
    qo, ko, vo = _run_tok_mlp(ops, d, do_mlp)
    D, D1 = (R.tok_mlp(*R.tok_mlp_args(d, do_mlp, r)) for r in (R.ident, R.bf1))
    outs = [("queries", qo[:P * T].reshape(P, T, 256), D[0], D1[0])]
    _guard_kept(qo, P * T, "queries_out")
    if do_mlp:
        outs += [("k", ko[:P * T].reshape(P, T, 128), D[1], D1[1]), ("v", vo[:P * T].reshape(P, T, 128), D[2], D1[2])]
        _guard_kept(ko, P * T, "k_out"); _guard_kept(vo, P * T, "v_out")
    else:
        assert bool((ko == SENT).all()) and bool((vo == SENT).all()), "do_mlp 0 wrote k_out / v_out"
    return _two_term(outs, what)


@pytest.mark.parametrize("P", R.TOK_P)
@pytest.mark.parametrize("T", R.TOK_T)
def test_dec_tok_mlp_against_float64(ops, P, T):
    """do_mlp 1 (three outputs) and do_mlp 0 with qpe, k_out, v_out and every MLP operand NULL (only queries_out is written).
    Measured worst err / limit over the twelve (P, T): max 0.141, rms 0.123."""
    d = R.to(R.tok_mlp_case(P, T), DEV)
    worst = max(_check_tok_mlp(ops, d, 1, f"dec_tok_mlp P={P} T={T} do_mlp=1"), _check_tok_mlp(ops, d, 0, f"dec_tok_mlp P={P} T={T} do_mlp=0"))
    print(f"dec_tok_mlp P={P} T={T}: worst err / limit {worst:.3f}")


def test_dec_tok_mlp_null_biases_and_layernorm_parameters(ops):
    """every bias and LayerNorm parameter NULL, both forms.  Measured worst err / limit: max 0.094, rms 0.097."""
    d = R.to(R.tok_mlp_special("nulls"), DEV)
    _check_tok_mlp(ops, d, 1, "dec_tok_mlp nulls do_mlp=1")
    _check_tok_mlp(ops, d, 0, "dec_tok_mlp nulls do_mlp=0")


def test_dec_tok_mlp_rows_whose_hidden_units_are_all_negative(ops):
    """b1 = -100 under |lin1| of a few units: ReLU gives zeros, lin2 contributes its bias only -- queries' = norm3(norm2(..) + b2).
    Measured worst err / limit: max 0.098, rms 0.093."""
    d = R.to(R.tok_mlp_special("dead"), DEV)
    y = R.tok_mlp(*R.tok_mlp_args(d, 0))[0]
    assert float((R.linear(y, d["W1"], d["b1"])).max()) < -50.0
    want = R.layer_norm(y + d["b2"].double(), d["ln3_w"], d["ln3_b"], d["eps"])
    assert float((R.tok_mlp(*R.tok_mlp_args(d, 1))[0] - want).abs().max()) < 1e-12
    _check_tok_mlp(ops, d, 1, "dec_tok_mlp dead hidden layer")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# dec_heads
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _run_heads(ops, hs, chains, m0, nm, n_iou):
    """-> (hyper buffer [P * nm + GUARD, 32], iou buffer flat [P * n_iou + 8]) prefilled with the sentinel"""
    P, T, _ = hs.shape
    keep = [ops.pack_mfma_rows(W) for ch in chains for W, _ in ch]             # the last weights are zero-padded to 16 rows here
    w_ptrs = torch.tensor([t.data_ptr() for t in keep], dtype=torch.int64)
    b_ptrs = torch.tensor([0 if b is None else b.data_ptr() for ch in chains for _, b in ch], dtype=torch.int64)      # (a None bias = NULL)
    hyper = _out(P * nm, 32)
    iou = torch.full((P * n_iou + 8,), SENT, device=DEV)
    _call("ullsam_dec_heads", hs.data_ptr(), w_ptrs.data_ptr(), b_ptrs.data_ptr(), hyper.data_ptr(), iou.data_ptr(), P, T, n_iou, m0, nm)
    return hyper, iou


@pytest.mark.parametrize("case", R.HEADS_CASES)
def test_dec_heads_against_float64(ops, case):
    """P in {1, 16, 17, 33} (one column, a full tile, one and two prompts into the next workgroup), T in {5, 7, 16} (the token stride; the IoU token is row 0),
    mask ranges (m0, nm) and n_iou in {4, 1}; hyper and iou are prefilled: exactly P nm 32 and P n_iou values change.  Measured worst err / limit over the six cases: max 0.160, rms 0.113."""
    P, T, m0, nm, n_iou = case
    hs, chains = R.to(R.heads_case(P, T, n_iou), DEV)
    hyper, iou = _run_heads(ops, hs, chains, m0, nm, n_iou)
    assert int((hyper != SENT).sum()) == P * nm * 32 and int((iou != SENT).sum()) == P * n_iou
    _guard_kept(hyper, P * nm, "hyper")
    assert bool((iou[P * n_iou:] == SENT).all())
    D, D1 = (R.heads(hs, chains, m0, nm, n_iou, r) for r in (R.ident, R.bf1))
    _two_term([("hyper", hyper[:P * nm].reshape(P, nm, 32), D[0], D1[0]), ("iou", iou[:P * n_iou].reshape(P, n_iou), D[1], D1[1])], f"dec_heads {case}")


@pytest.mark.parametrize("chain", R.HEADS_NULL_CHAINS)
def test_dec_heads_chain_with_null_biases(ops, chain):
    """one hypernetwork chain / the IoU chain with its three biases NULL.  Measured worst err / limit: max 0.088, rms 0.095."""
    hs, ch0 = R.to(R.heads_null_case(chain), DEV)
    P, T, _ = hs.shape
    hyper, iou = _run_heads(ops, hs, ch0, 0, 4, 4)
    D, D1 = (R.heads(hs, ch0, 0, 4, 4, r) for r in (R.ident, R.bf1))
    _two_term([("hyper", hyper[:P * 4].reshape(P, 4, 32), D[0], D1[0]), ("iou", iou[:P * 4].reshape(P, 4), D[1], D1[1])], f"dec_heads null biases of chain {chain}")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# batch independence of the token kernels and the heads, bitwise
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_token_kernels_do_not_depend_on_the_batch(ops):
    """prompt p alone gives the bits it has inside a batch of three (one workgroup per prompt, fixed summation order): dec_tok_attn, dec_tok_mlp"""
    P, T = 3, 7
    d = R.to(R.tok_attn_case(P, T, seed=3), DEV)
    qo, q2 = _run_tok_attn(ops, d, 0, 0)
    m = R.to(R.tok_mlp_case(P, T, seed=3), DEV)
    mo, ko, vo = _run_tok_mlp(ops, m, 1)
    for p in range(P):
        one = dict(d, queries=d["queries"][p:p + 1].contiguous(), qpe=d["qpe"][p:p + 1].contiguous())
        qo1, q21 = _run_tok_attn(ops, one, 0, 0)
        assert torch.equal(qo1[:T], qo[p * T:(p + 1) * T]) and torch.equal(q21[:T], q2[p * T:(p + 1) * T])
        one = dict(m, queries=m["queries"][p:p + 1].contiguous(), attn=m["attn"][p:p + 1].contiguous(), qpe=m["qpe"][p:p + 1].contiguous())
        mo1, ko1, vo1 = _run_tok_mlp(ops, one, 1)
        assert torch.equal(mo1[:T], mo[p * T:(p + 1) * T]) and torch.equal(ko1[:T], ko[p * T:(p + 1) * T]) and torch.equal(vo1[:T], vo[p * T:(p + 1) * T])


def test_dec_heads_do_not_depend_on_the_batch_or_on_poisoned_neighbours(ops):
    """the same prompt at batch positions 0, 5 and 17 (other MFMA columns, another workgroup) and alone has the same bits; and still the same when ANOTHER prompt
    of its group of 16 holds Inf / NaN tokens: the MFMA's columns are independent, poison must not cross."""
    P, T = 33, 7
    hs, chains = R.to(R.heads_case(P, T, 4, seed=2), DEV)
    hs[5] = hs[0]; hs[17] = hs[0]
    hyper, iou = _run_heads(ops, hs, chains, 0, 4, 4)
    h1, i1 = _run_heads(ops, hs[:1].contiguous(), chains, 0, 4, 4)
    hyper, iou = hyper[:P * 4].reshape(P, 4, 32), iou[:P * 4].reshape(P, 4)
    for p in (0, 5, 17):
        assert torch.equal(hyper[p], h1[:4]) and torch.equal(iou[p], i1[:4]), p
    bad = hs.clone()
    bad[3, :, ::2] = float("inf"); bad[3, :, 1::2] = float("nan"); bad[20] = float("-inf")
    hb, ib = _run_heads(ops, bad, chains, 0, 4, 4)
    hb, ib = hb[:P * 4].reshape(P, 4, 32), ib[:P * 4].reshape(P, 4)
    ok = [p for p in range(P) if p not in (3, 20)]
    assert torch.equal(hb[ok], hyper[ok]) and torch.equal(ib[ok], iou[ok])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# i2t_block
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _run_i2t(d, P, N, T, shared, want=(True, True, True)):
    """-> (out_f32, out_c, out_c_pe) buffers with guard rows (None where not requested)"""
    rows = P * N
    of = _out(rows, 256) if want[0] else None
    oc = _out(rows, 256, torch.bfloat16) if want[1] else None
    op = _out(rows, 256, torch.bfloat16) if want[2] else None
    mod = N if shared else 0
    assert d["xin"].shape[0] == (1 if shared else P) and d["ktok"].shape == (P, T, 128)
    _call("ullsam_i2t_block", d["xin"].data_ptr(), mod, d["res"].data_ptr(), mod, d["Wq"].data_ptr(), _p(d["bq"]), d["ktok"].data_ptr(), d["vtok"].data_ptr(),
          d["Wo"].data_ptr(), _p(d["bo"]), _p(d["lnw"]), _p(d["lnb"]), float(d["eps"]), d["key_pe"].data_ptr(), N, _p(of), _p(oc), _p(op), P, T, N, float(d["scale"]))
    return of, oc, op


def _i2t_consistent(d, of, oc, op, P, N):
    """the three outputs against each other, exact: out_c = bf16(out_f32), out_c_pe = bf16(out_f32 + key_pe[row % N]); sentinel rows kept"""
    rows = P * N
    for b, n in ((of, "out_f32"), (oc, "out_c"), (op, "out_c_pe")):
        _guard_kept(b, rows, n)
    assert torch.equal(oc[:rows], of[:rows].bfloat16())
    assert torch.equal(op[:rows], (of[:rows].reshape(P, N, 256) + d["key_pe"][None]).reshape(rows, 256).bfloat16())


def _check_i2t(d, P, N, T, shared, what, flips=True):
    of, oc, op = _run_i2t(d, P, N, T, shared)
    _i2t_consistent(d, of, oc, op, P, N)
    got = of[:P * N].reshape(P, N, 256)
    D = R.i2t(*R.i2t_args(d))
    ratio = _within(got, D, R.i2t_bound(d, flips=flips), what)
    if flips and T > 1:                   # (T = 1 and the selection inputs: D1 = D, nothing to scale an rms limit with; their element bound is the fp32 one)
        (em, er), (lm, lr) = R.err(got, D), R.err(R.i2t(*R.i2t_args(d, R.bf1)), D)
        print(f"{what}: rms {er:.2e}, limit {lr / 8:.2e}: {er / (lr / 8):.3f}; max {em:.2e} (D1: {lm:.2e})")
        assert er <= lr / 8, (what, er, lr / 8)
    return got, D, ratio


@pytest.mark.parametrize("case", R.I2T_CASES)
def test_i2t_block_against_float64(case):
    """(P, N) = (1, 5): one partial group, seven idle waves; (3, 200): two workgroups per prompt, idle waves, 8 live rows in the last group; (257, 275):
    one workgroup per prompt, waves of three and two trips, N % 16 = 3; (64, 1024): the smallest production-gated shape, two trips; T in {1, 4, 5, 15, 16}; the
    shared-image and the per-prompt form.  rms(got - D) <= rms(D1 - D) / 8, every element inside decoder_ref.i2t_bound, the three outputs consistent, sentinel rows
    kept.  Measured over the nine cases: rms / limit <= 0.319, worst element err / bound <= 0.100 (the bound lets EVERY element of the cast step at once)."""
    P, N, T, shared = case
    d = R.to(R.i2t_case(P, N, T, shared), DEV)
    got, D, _ = _check_i2t(d, P, N, T, shared, f"i2t_block {case}")
    if T == 1:                            # one token: every arithmetic gives the definition (softmax = 1, a = v); the element bound has been applied
        assert R.err(R.i2t(*R.i2t_args(d, R.bf1)), D) == (0.0, 0.0)


def test_i2t_block_every_combination_of_outputs():
    """each of the eight subsets of (out_f32, out_c, out_c_pe): a requested output has the bits of the all-three launch (out_c the same when out_f32 is not
    requested), guard rows kept"""
    P, N, T = 3, 200, 5
    d = R.to(R.i2t_case(P, N, T, False, seed=1), DEV)
    full = _run_i2t(d, P, N, T, False)
    _i2t_consistent(d, *full, P, N)
    for want in itertools.product((False, True), repeat=3):
        outs = _run_i2t(d, P, N, T, False, want)
        for w, o, f in zip(want, outs, full):
            assert (o is None) == (not w)
            if w:
                assert torch.equal(o, f), want


def test_i2t_block_null_biases_and_layernorm_parameters():
    """bq, bo, lnw, lnb NULL.  Measured: rms / limit 0.236, worst element err / bound 0.030."""
    P, N, T, shared = R.I2T_SPECIAL["nulls"]
    d = R.to(R.i2t_special("nulls"), DEV)
    _check_i2t(d, P, N, T, shared, "i2t_block nulls")


@pytest.mark.parametrize("name", ["offset50", "offset200"])
def test_i2t_block_residual_with_a_large_common_offset(name):
    """res = keys + 50 / + 200 (row mean ~ offset, spread ~1): norm4's variance has to be two-pass; the element bound scales with |res| through its fp32 term.
    At 50 a one-pass variance (E[x^2] - mean^2 in fp32) with the best summation order still fits the rms limit; at 200 it loses 16x more and breaks it
    (rms 6x over: asserted on a restatement in test_decoder_ref_cpu.py), while the legitimate fp32 roundings of a sum near 200 (2^-17 = 8e-6 each) stay inside.
    Measured: offset 50: rms / limit 0.216, worst element err / bound 0.036; offset 200: rms / limit 0.226, worst element err / bound 0.034."""
    P, N, T, shared = R.I2T_SPECIAL[name]
    d = R.to(R.i2t_special(name), DEV)
    assert abs(float(d["res"].mean()) - float(name[6:])) < 0.1
    _check_i2t(d, P, N, T, shared, f"i2t_block {name}")


@pytest.mark.parametrize("T", [1, 5, 16])
def test_i2t_block_exact_selection(T):
    """inputs whose softmax selects one token per (row, head) (decoder_ref.i2t_selection_case; the margins are asserted in test_decoder_ref_cpu.py): the
    attention output is the winner's bf16 value, its cast cannot flip, and the fp32-level bound (decoder_ref.i2t_bound without the flip term) holds for every
    element -- this pins the q projection, the score product, the masking of tokens >= T (an unmasked one would win) and the head -> column map.  T = 1: the
    result does not depend on q at all -- other image rows give the same bits.  Besides the derived bound (worst case of 130 fp32 roundings: loose, measured
    err / bound 0.006) every element is held to the project's bound for fp32 LayerNorm chains, 2e-5 absolute (test_kernels_gpu.py); measured max |err| 1.2e-6:
    0.06 of it."""
    P, N = 2, 200
    d, win = R.i2t_selection_case(P, N, T)
    d = R.to(d, DEV)
    got, D, _ = _check_i2t(d, P, N, T, False, f"i2t_block selection T={T}", flips=False)
    _within(got, D, 2e-5, f"i2t_block selection T={T}, 2e-5")
    if T == 1:
        other = dict(d, xin=R.to(R.i2t_case(P, N, T, False, seed=9)["xin"], DEV))
        of, oc, op = _run_i2t(other, P, N, T, False)
        assert not torch.equal(other["xin"], d["xin"]) and torch.equal(of[:P * N].reshape(P, N, 256), got)
    else:
        a = R.i2t(*R.i2t_args(d, R.ident, True, True))[2].reshape(P, N, 8, 16)
        v = d["vtok"].double().reshape(P, T, 8, 16)
        pick = torch.gather(v.transpose(1, 2)[:, None].expand(P, N, 8, T, 16), 3, win.to(DEV)[..., None, None].expand(P, N, 8, 1, 16)).squeeze(3)
        assert torch.equal(a, pick)          # the definition's attention output IS the drawn winner's value


def test_i2t_block_does_not_depend_on_the_batch():
    """prompt 0's three outputs from a P = 1 launch (53 workgroups for its 6700 rows) equal its outputs inside P = 5 (52 workgroups per prompt: another
    assignment of row groups to waves), bitwise; and the shared-image launch equals the per-prompt launch on replicated inputs."""
    P, N, T = 5, 6700, 7
    d = R.to(R.i2t_case(P, N, T, False, seed=4), DEV)
    assert -(-(-(-N // 16)) // 8) == 53 and -(-256 // P) == 52
    full = _run_i2t(d, P, N, T, False)
    one = dict(d, xin=d["xin"][:1].contiguous(), res=d["res"][:1].contiguous(), ktok=d["ktok"][:1].contiguous(), vtok=d["vtok"][:1].contiguous())
    for a, b in zip(_run_i2t(one, 1, N, T, False), full):
        assert torch.equal(a[:N], b[:N])
    P, N = 3, 200
    s = R.to(R.i2t_case(P, N, T, True, seed=5), DEV)
    rep = dict(s, xin=s["xin"].expand(P, -1, -1).contiguous(), res=s["res"].expand(P, -1, -1).contiguous())
    for a, b in zip(_run_i2t(s, P, N, T, True), _run_i2t(rep, P, N, T, False)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# kv_proj, up1_ln_gelu, up2_hyper_masks
# ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [1, 15, 2049 * 16 + 1])
def test_kv_proj_against_float64(rows):
    """one row, one partial group, and 2050 groups = two more than the 256 workgroups x 8 waves take in one trip (the second trip's ragged end); biases given, then
    bk NULL with bv given; guard rows.  Measured worst err / bound: 0.98 (2^-8 |ref| is the worst case of the one rounding itself: a correct kernel reaches it)."""
    d = R.to(R.kv_case(rows), DEV)
    for bk in (d["bk"], None):
        K, V = _out(rows, 128, torch.bfloat16), _out(rows, 128, torch.bfloat16)
        _call("ullsam_kv_proj", d["xk"].data_ptr(), d["xv"].data_ptr(), d["Wk"].data_ptr(), d["Wv"].data_ptr(), _p(bk), d["bv"].data_ptr(), K.data_ptr(), V.data_ptr(), rows)
        Kd, Vd = R.kv_proj(d["xk"], d["xv"], d["Wk"], bk, d["Wv"], d["bv"])
        _within(K[:rows], Kd, R.kv_bound(d["xk"], d["Wk"], bk, Kd), f"kv_proj K rows={rows} bk={'given' if bk is not None else 'NULL'}")
        _within(V[:rows], Vd, R.kv_bound(d["xv"], d["Wv"], d["bv"], Vd), f"kv_proj V rows={rows}")
        _guard_kept(K, rows, "K"); _guard_kept(V, rows, "V")


@pytest.mark.parametrize("rows", [1, 5, 1000, 65557])
def test_up1_ln_gelu_against_float64(rows):
    """rows % 4 != 0 (the store gate on row0 + e), and 65557 rows = 4098 groups: the first launch whose waves take more than one trip (256 workgroups x 8 waves
    = 2048 groups per trip), with a ragged end; guard rows.  Measured worst err / bound: 0.92 (the rounding itself, as for kv_proj)."""
    d = R.to(R.up1_case(rows), DEV)
    out = _out(rows * 4, 64, torch.bfloat16)
    _call("ullsam_up1_ln_gelu", d["src"].data_ptr(), d["w0"].data_ptr(), d["b0"].data_ptr(), d["lnw"].data_ptr(), d["lnb"].data_ptr(), float(d["eps"]), out.data_ptr(), rows)
    want = R.up1(d["src"], d["w0"], d["b0"], d["lnw"], d["lnb"], d["eps"])
    _within(out[:rows * 4], want, R.up1_bound(d, d["b0"], d["lnw"], d["lnb"], want), f"up1_ln_gelu rows={rows}")
    _guard_kept(out, rows * 4, "up1 out")


def test_up1_ln_gelu_null_parameters_and_a_zero_row():
    """b0, lnw, lnb NULL; then b0 NULL with an all-zero source row: its four taps have variance 0 and the output is gelu(lnb) (to the bf16 rounding), finite.
    Measured worst err / bound: 0.89, zero row 0.94."""
    rows = 21
    d = R.up1_case(rows, seed=1)
    d["src"][7] = 0
    d = R.to(d, DEV)
    for lnw, lnb in ((None, None), (d["lnw"], d["lnb"])):
        out = _out(rows * 4, 64, torch.bfloat16)
        _call("ullsam_up1_ln_gelu", d["src"].data_ptr(), d["w0"].data_ptr(), None, _p(lnw), _p(lnb), float(d["eps"]), out.data_ptr(), rows)
        want = R.up1(d["src"], d["w0"], None, lnw, lnb, d["eps"])
        _within(out[:rows * 4], want, R.up1_bound(d, None, lnw, lnb, want), "up1_ln_gelu nulls")
        _guard_kept(out, rows * 4, "up1 out")
        g = R.gelu(lnb.double()) if lnb is not None else torch.zeros(64, dtype=torch.float64, device=DEV)
        assert float((want[28:32] - g).abs().max()) == 0.0
        _within(out[28:32], g[None].expand(4, -1), R.bf16_bound(g[None].expand(4, -1), 1.9e-6 + 4 * R.U24), "up1_ln_gelu zero row")


@pytest.mark.parametrize("case", [(2, 3, 5, 8), (1, 6, 10, 3), (3, 64, 64, 4)])
def test_up2_hyper_masks_against_float64(case):
    """(NB, H, W, NM): non-square grids (the (y, x) decode from pix / W), a partial last group (3 x 5 x 4 = 60 rows), waves of three and four trips leaving
    through both breaks of the two-buffer loop (64 x 64: 1024 groups over 64 workgroups x 4 waves = 4 trips; 6 x 10: 15 groups, one workgroup: 4, 4, 4, 3
    trips), NM = 8; b1 given and NULL; a guard plane behind the output.  Measured worst err / bound: 0.65."""
    NB, H, W, NM = case
    d = R.to(R.up2_case(NB, H, W, NM), DEV)
    for b1 in (d["b1"], None):
        out = torch.full((NB * NM + 1, 4 * H, 4 * W), SENT, device=DEV)
        _call("ullsam_up2_hyper_masks", d["u1"].data_ptr(), d["w1"].data_ptr(), _p(b1), d["hyper"].data_ptr(), out.data_ptr(), NB, NM, H, W)
        want = R.up2(d["u1"], d["w1"], b1, d["hyper"], NB, NM, H, W, cast=False)
        _within(out[:NB * NM].reshape(NB, NM, 4 * H, 4 * W), want, R.up2_bound(d, b1, NB, NM, H, W), f"up2_hyper_masks {case} b1={'given' if b1 is not None else 'NULL'}")
        assert bool((out[NB * NM] == SENT).all()) and not bool((out[:NB * NM] == SENT).any())
