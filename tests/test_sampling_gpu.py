"""The seeded fused sampler (ullsam_sample_topk_topp, csrc/llm_misc.hip) against its float64 definition (tests/sampling_ref.py), its device Philox
against the host mirror (ullsam_amd/sampling.py), its draws as frequencies, and generate(seed=...) on the tiny fp32 model.

Tolerances: candidate ids are exact (the order is total: value descending, id ascending).  Probabilities: 1e-5 absolute (fp32 exp / sums of at most
1024 terms in blocks of 16 and a 64-lane tree against float64).  Draws: eps = 4 * top_k * 2^-24 on the cumulative boundaries (sampling_ref.eps_for)."""
import numpy as np
import pytest
import torch

from tests import sampling_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24
VS = [1, 7, 64, 1000, 1025, 4097, 92553]
KS = [1, 2, 50, 64, 65, 256, 1024]
TPS = [(0.7, 0.9), (1.0, 1.0), (1.3, 0.5)]
ROW_NAMES = ["random0", "random1", "random2", "peaked", "halves", "equal", "max0", "maxlast", "tie1", "tie64", "tie1024", "tie4096", "tie_cross",
             "plateau", "zeros", "three_finite", "neginf", "posinf", "nan_some", "nan_all"]
NAN_ROWS = [ROW_NAMES.index("nan_some"), ROW_NAMES.index("nan_all")]


@pytest.fixture(scope="module")
def ops():
    from ullsam_amd import ops as o
    return o


def _s():
    return torch.cuda.current_stream().cuda_stream


def sampler_rows(V):
    """fp32 rows [20, V] (CPU).  random x3 (sigma 3); peaked (one logit 30 above the rest); halves (rounded to multiples of 0.5: many exact ties, also at
    the k-th value); equal; maximum at 0 / at V - 1; ties of the two top values (the row's maximum + 1) in the pairs of places the kernel treats differently -- neighbouring lanes
    (i, i + 1), different waves (i, i + 64), one thread's unroll slots (i, i + 1024), one thread's trips (i, i + 4096), different trips with the LATER id
    in the LOWER thread (5, 4096 + 3); plateau (ten distinct values above a row of 1.25: more values equal to the k-th than sort slots, the id-ordered
    tie scan with candidates above it; `equal` is that scan with none above); zeros (-0.0 and 0.0 on top: equal values, id order); -inf in all but three
    places; all -inf; one +inf... NaN in every third place; all NaN.  A pair whose second member does not fit into V leaves its row random."""
    g = torch.Generator(); g.manual_seed(1000 + V)
    x = torch.randn((len(ROW_NAMES), V), generator=g) * 3.0
    n = {name: i for i, name in enumerate(ROW_NAMES)}
    x[n["peaked"], (V * 2) // 3] = x[n["peaked"]].max() + 30.0
    x[n["halves"]] = torch.round(x[n["halves"]]) / 2
    x[n["equal"]] = 1.25
    top = lambda name: float(x[n[name]].max()) + 1.0                       # (one above the rest, not far above: the rest keeps a mass the draws can land in)
    x[n["max0"], 0] = top("max0")
    x[n["maxlast"], V - 1] = top("maxlast")
    t1024 = (0, 1024) if V <= 1027 else (3, 3 + 1024)
    t4096 = (0, 4096) if V <= 4105 else (9, 9 + 4096)
    for name, (i, j) in (("tie1", (10, 11)), ("tie64", (17, 17 + 64)), ("tie1024", t1024), ("tie4096", t4096), ("tie_cross", (5, 4096 + 3))):
        if j < V:
            x[n[name], i] = x[n[name], j] = top(name)
    x[n["plateau"]] = 1.25
    for t in range(min(10, V - 1)):
        x[n["plateau"], (t * 7919 + 1) % V] = 2.0 + 0.37 * t            # (places that coincide at a small V just leave fewer than ten)
    x[n["zeros"]] = -x[n["zeros"]].abs() - 1.0
    for t, i in enumerate([2, 5, 9, 1030, 4100]):
        if i < V:
            x[n["zeros"], i] = -0.0 if t % 2 else 0.0
    x[n["three_finite"]] = float("-inf")
    for t, i in enumerate([V // 5, V // 2, V - 1]):
        x[n["three_finite"], i] = 0.3 * t - 0.2
    x[n["neginf"]] = float("-inf")
    x[n["posinf"], V // 3] = float("inf")
    if V > 2:
        x[n["posinf"], V - 1] = float("inf")                               # a second one: the FIRST +inf is the answer
    x[n["nan_some"], ::3] = float("nan")
    x[n["nan_all"]] = float("nan")
    return x


_CACHE = {}


def rows_and_orders(V):
    """The rows of sampler_rows(V) and each row's full order (sampling_ref.full_order), computed once per V and shared read-only."""
    if V not in _CACHE:
        x = sampler_rows(V)
        xn = x.numpy()
        xn.setflags(write=False)
        _CACHE[V] = (x, [R.full_order(xn[r]) for r in range(x.shape[0])])
    return _CACHE[V]


def _raw_call(buf, V, T, k, p, seeds, step, u):
    """The C entry directly on a [R, ld] buffer (ld = buf.shape[1] >= V) -> (ids, u_out, cand_ids, cand_p); one slot more than needed behind each
    output holds a sentinel that must survive."""
    from ullsam_amd import _lib
    Rn, ld = buf.shape
    out = torch.full((Rn + 1,), -77, dtype=torch.int64, device=DEV)
    u_out = torch.full((Rn + 1,), -77.0, dtype=torch.float32, device=DEV)
    ci = torch.full((Rn * k + 1,), -77, dtype=torch.int64, device=DEV)
    cp = torch.full((Rn * k + 1,), -77.0, dtype=torch.float32, device=DEV)
    _lib.call("ullsam_sample_topk_topp", buf.data_ptr(), out.data_ptr(), Rn, V, ld, float(T), int(k), float(p), seeds.data_ptr(), int(step),
              None if u is None else u.data_ptr(), u_out.data_ptr(), ci.data_ptr(), cp.data_ptr(), _s())
    out, u_out, ci, cp = out.cpu(), u_out.cpu(), ci.cpu(), cp.cpu()
    assert int(out[Rn]) == -77 and float(u_out[Rn]) == -77.0 and int(ci[Rn * k]) == -77 and float(cp[Rn * k]) == -77.0
    return out[:Rn], u_out[:Rn], ci[:Rn * k].reshape(Rn, k), cp[:Rn * k].reshape(Rn, k)


def _check_candidates(name, ref, k, p, ids_row, p_row):
    kk = len(ref["ids"])
    eps = R.eps_for(k)
    assert ids_row[:kk].tolist() == ref["ids"].tolist(), name                 # the deterministic tie rule: exact
    assert bool((ids_row[kk:] == -1).all()) and bool((p_row[kk:] == 0).all()), name
    got, want = p_row[:kk].astype(np.float64), ref["probs"]
    amb = [j for j in range(1, kk) if p < 1.0 and abs(ref["before"][j] - p) <= eps]
    if not amb:
        assert np.abs(got - want).max() < 1e-5, (name, float(np.abs(got - want).max()))
        return
    # a candidate within eps of the nucleus boundary may be kept or dropped; everything in front of the first such one must agree, and the
    # probabilities are compared after renormalising over the common kept set
    j0 = min(amb)
    assert ((got[:j0] > 0) == (want[:j0] > 0)).all(), name
    common = (got > 0) & (want > 0)
    assert common[0]
    assert np.abs(got[common] / got[common].sum() - want[common] / want[common].sum()).max() < 1e-5, name


@pytest.mark.parametrize("V", VS)
def test_kernel_against_the_definition(ops, V):
    """Every top_k of KS (also top_k > V) x every (T, top_p) of TPS on the 20 rows of sampler_rows(V), through the wrapper (ld = V) and through the raw
    entry with ld = V + 5 and LARGER values (1e9) in the pad columns: candidate ids exact for NaN-free rows, probabilities within 1e-5 (candidates
    within eps of the nucleus boundary: either reading), the drawn id one of the tokens sampling_ref.accepted allows for the u the kernel reports;
    NaN rows: only 0 <= id < V."""
    from ullsam_amd import sampling
    x, orders = rows_and_orders(V)
    Rn = x.shape[0]
    xd = x.to(DEV)
    buf = torch.full((Rn, V + 5), 1e9)
    buf[:, :V] = x
    bd = buf.to(DEV)
    seeds_np = sampling.row_seeds(77 + V, Rn)
    seeds = torch.from_numpy(seeds_np.view(np.int64)).to(DEV)
    for ik, k in enumerate(KS):
        for it, (T, p) in enumerate(TPS):
            step = 3 * ik + it
            refs = [R.reference(x[r].numpy(), T, k, p, order=orders[r]) for r in range(Rn)]
            a = ops.sample_topk_topp(xd, T, k, p, seeds, step, return_debug=True)
            b = _raw_call(bd, V, T, k, p, seeds, step, None)
            want_u = sampling.uniforms(seeds_np, step)
            for ids, u, ci, cp in (tuple(t.cpu() for t in a), b):
                ids, u, ci, cp = ids.numpy(), u.numpy(), ci.numpy(), cp.numpy()
                assert ci.shape == (Rn, k) and cp.shape == (Rn, k)
                assert bool(((ids >= 0) & (ids < V)).all()), ids.tolist()
                assert u.tobytes() == want_u.tobytes()
                for r in range(Rn):
                    if r in NAN_ROWS:
                        continue
                    name = (ROW_NAMES[r], V, k, T, p)
                    _check_candidates(name, refs[r], k, p, ci[r], cp[r])
                    assert int(ids[r]) in R.accepted(refs[r], float(u[r]), R.eps_for(k)), name
            assert a[0].cpu().tolist() == b[0].tolist()                       # the stride changes nothing


def _draw_us(ref, eps):
    """The u values of the draw test for one row: six fixed ones, then just below / just above (adjacent fp32 values) three interior boundaries of the
    reference CDF (first, middle, last; 0.5 where the row has fewer).  Only boundaries between two candidates that each weigh more than 2 eps are
    taken, so that the interval widened by eps reaches no third candidate."""
    fixed = [0.0, U24, 0.25, 0.5, 0.9, 1.0 - U24]
    pr = ref["probs"]
    c = np.cumsum(pr)
    inner = [float(c[j]) for j in range(len(c) - 1) if pr[j] > 2 * eps and pr[j + 1] > 2 * eps and 4 * U24 < c[j] < 1.0 - 4 * U24]
    inner = sorted(set(inner))
    pick = [inner[0], inner[len(inner) // 2], inner[-1]] if inner else []
    edge = []
    for v in pick:
        f = np.float32(v)
        edge += [float(np.nextafter(f, np.float32(-1))), float(np.nextafter(f, np.float32(2)))]
    edge += [0.5] * (6 - len(edge))
    return fixed, edge


@pytest.mark.parametrize("V", [1000, 4097, 92553])
def test_draws_with_explicit_u(ops, V):
    """The drawn id for a GIVEN u, per row: u in {0, 2^-24, 0.25, 0.5, 0.9, 1 - 2^-24} and the fp32 neighbours of three interior boundaries of the
    reference CDF, for (top_k, T, top_p) in {(50, 0.7, 0.9), (64, 1.0, 1.0), (5, 1.3, 0.5)}.  The id must be in accepted(ref, u, eps).  So that the
    widening by eps cannot hide a wrong draw, the accepted set is a SINGLE token in at least 90 % of the (row, fixed u) cases -- checked here on the CPU
    before the kernel runs (V >= 1000 so that top_k cuts the tail off: with the whole vocabulary as candidates the last ones weigh less than eps and
    u = 1 - 2^-24 accepts several of them).  The share is taken over the six FIXED u of each row, not over all twelve: the six boundary neighbours lie
    one fp32 step from a boundary, closer than eps, so each accepts the token on either side by construction and a share over all (row, u) cases could
    not reach 90 % with this set of u.  For those cases it is asserted instead that at most two tokens are accepted (the boundaries are taken between
    candidates heavier than 2 eps), so the widening hides no more than the one neighbour there, and the kernel must return one of the two."""
    x, orders = rows_and_orders(V)
    Rn = x.shape[0]
    xd = x.to(DEV)
    seeds = torch.zeros((Rn,), dtype=torch.int64, device=DEV)
    clean = [r for r in range(Rn) if r not in NAN_ROWS]
    for k, T, p in ((50, 0.7, 0.9), (64, 1.0, 1.0), (5, 1.3, 0.5)):
        eps = R.eps_for(k)
        refs = [R.reference(x[r].numpy(), T, k, p, order=orders[r]) for r in range(Rn)]
        us = [sum(_draw_us(refs[r], eps), []) for r in range(Rn)]              # [Rn][12]
        single = sum(len(R.accepted(refs[r], us[r][i], eps)) == 1 for r in clean for i in range(6))
        assert single >= 0.9 * 6 * len(clean), (V, k, single)
        assert all(len(R.accepted(refs[r], us[r][i], eps)) <= 2 for r in clean for i in range(6, 12)), (V, k)
        for i in range(12):
            u_np = np.array([us[r][i] for r in range(Rn)], dtype=np.float32)
            assert bool(((u_np >= 0) & (u_np < 1)).all())
            ids, u_back, _, _ = ops.sample_topk_topp(xd, T, k, p, seeds, 0, u=torch.from_numpy(u_np).to(DEV), return_debug=True)
            ids = ids.cpu().numpy()
            assert u_back.cpu().numpy().tobytes() == u_np.tobytes()
            assert bool(((ids >= 0) & (ids < V)).all())
            for r in clean:
                acc = R.accepted(refs[r], float(u_np[r]), eps)
                assert int(ids[r]) in acc, (ROW_NAMES[r], V, k, float(u_np[r]), int(ids[r]), sorted(acc))


def test_device_rng_matches_the_host_mirror(ops):
    """u_in = NULL: u_out equals sampling.uniforms(seeds, step) bit for bit (seeds 0, 1, 2^32, 2^64 - 1 among them; steps 0, 1, 2^32 + 5), the ids
    equal those of a call that is handed that u, and a repeated call gives the same ids."""
    from ullsam_amd import sampling
    seeds_np = np.array([0, 1, 2 ** 32, 2 ** 64 - 1, 2 ** 63, 0x0123456789ABCDEF, 42, 2 ** 32 - 1], dtype=np.uint64)
    g = torch.Generator(); g.manual_seed(5)
    x = (torch.randn((len(seeds_np), 1000), generator=g) * 2.0).to(DEV)
    seeds = torch.from_numpy(seeds_np.view(np.int64)).to(DEV)
    seen = set()
    for step in (0, 1, 2 ** 32 + 5):
        ids, u, _, _ = ops.sample_topk_topp(x, 0.7, 50, 0.9, seeds, step, return_debug=True)
        want = sampling.uniforms(seeds_np, step)
        assert u.cpu().numpy().tobytes() == want.tobytes(), (step, u.cpu().tolist(), want.tolist())
        again = ops.sample_topk_topp(x, 0.7, 50, 0.9, seeds, step)
        given = ops.sample_topk_topp(x, 0.7, 50, 0.9, seeds, step, u=torch.from_numpy(want).to(DEV))
        assert ids.cpu().tolist() == again.cpu().tolist() == given.cpu().tolist()
        seen.add(tuple(ids.cpu().tolist()))
    assert len(seen) == 3                                                    # the step moves the draws (8 rows x ~50 tokens: equal only by a bug)


def test_argument_errors(ops):
    from ullsam_amd import _lib
    x = torch.zeros((2, 100), device=DEV)
    seeds = torch.zeros((2,), dtype=torch.int64, device=DEV)
    for T, k, p in ((0.7, 0, 0.9), (0.7, 1025, 0.9), (0.0, 50, 0.9), (-1.0, 50, 0.9), (0.7, 50, 0.0)):
        with pytest.raises(_lib.UllsamError):
            ops.sample_topk_topp(x, T, k, p, seeds, 0)


def test_frequencies_follow_the_probabilities(ops):
    """One row (V = 64, top_k = 8, T = 1, top_p = 0.9) repeated over 65536 rows with seeds 0 .. 65535: every candidate's frequency is within
    5 sqrt(p (1 - p) / N) of its reference probability, and the two candidates outside the nucleus (mass before them 0.93 and 0.97) and the 56 tokens
    outside the top 8 are never drawn.  Fixed seeds: the outcome is deterministic."""
    N, V, k = 65536, 64, 8
    probs = np.array([0.3, 0.2, 0.15, 0.12, 0.1, 0.06, 0.04, 0.03])
    places = [41, 3, 63, 0, 17, 30, 8, 55]
    row = np.full((V,), -9.0, np.float32)
    row[places] = np.log(probs).astype(np.float32)
    ref = R.reference(row, 1.0, k, 0.9)
    assert ref["ids"].tolist() == places and (ref["probs"] > 0).sum() == 6 and np.abs(ref["before"][1:] - 0.9).min() > 0.02
    x = torch.from_numpy(row).to(DEV).repeat(N, 1).contiguous()
    seeds = torch.arange(N, dtype=torch.int64, device=DEV)
    ids = ops.sample_topk_topp(x, 1.0, k, 0.9, seeds, 0).cpu().numpy()
    counts = np.bincount(ids, minlength=V)
    assert counts.sum() == N
    for j, tok in enumerate(places):
        q = ref["probs"][j]
        f = counts[tok] / N
        assert abs(f - q) <= 5 * np.sqrt(q * (1 - q) / N), (tok, f, q)
    assert counts[[8, 55]].sum() == 0 and counts.sum() == counts[places].sum()


# ---- generate(seed=...) on the tiny fp32 model ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lm():
    from tests.test_model_gpu import _tiny_llm
    return _tiny_llm(torch.float32)


IDS = [[1, 5, 9, 100, 7]]


def _gen(lm, seed, n=6, ids=IDS, **kw):
    kw.setdefault("eos_token_id", -1)
    kw.setdefault("temperature", 1.5)
    kw.setdefault("top_k", 50)
    t = torch.tensor(ids, device=DEV)
    return lm.generate(input_ids=t, max_new_tokens=n, do_sample=True, seed=seed, **kw)[:, t.shape[1]:].cpu().tolist()


def test_generate_seed_top_k_1_is_greedy(lm):
    t = torch.tensor(IDS, device=DEV)
    greedy = lm.generate(input_ids=t, max_new_tokens=4, eos_token_id=-1)
    sampled = lm.generate(input_ids=t, max_new_tokens=4, eos_token_id=-1, do_sample=True, seed=3, top_k=1, temperature=0.7, top_p=0.9)
    assert sampled.tolist() == greedy.tolist()


def test_generate_seed_reproduces_and_leaves_the_global_generator_alone(lm):
    torch.manual_seed(123)
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state()
    a = _gen(lm, 7, top_p=0.9)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(), gpu_state)
    torch.manual_seed(999)
    torch.rand(5, device=DEV); torch.rand(5)
    b = _gen(lm, 7, top_p=0.9)
    assert a == b
    t = torch.tensor(IDS, device=DEV)
    d = lm.generate(input_ids=t, generation_config={"max_new_tokens": 6, "do_sample": True, "seed": 7, "eos_token_id": -1}, temperature=1.5, top_k=50,
                    top_p=0.9)[:, 5:].cpu().tolist()
    assert d == a                                                            # (the seed read from a dict generation_config)
    assert _gen(lm, 7) != _gen(lm, 8)                                        # two seeds, T 1.5, top_k 50, 6 tokens: equal with probability ~ 50^-6 at best


def _recorded(lm, ops, monkeypatch, seed, **kw):
    """A seeded run with every step's (u, candidate probabilities) recorded -> (new tokens, smallest distance of a draw from a CDF boundary)."""
    real = ops.sample_topk_topp
    margin = []

    def spy(logits, T, k, p, seeds, step, u=None, return_debug=False):
        ids, uu, ci, cp = real(logits, T, k, p, seeds, step, return_debug=True)
        c = np.cumsum(cp.double().cpu().numpy(), -1)
        margin.append(float(np.abs(c - uu.double().cpu().numpy()[:, None]).min()))
        return ids

    with monkeypatch.context() as mp:
        mp.setattr(ops, "sample_topk_topp", spy)
        toks = lm.generate(do_sample=True, seed=seed, temperature=1.5, top_k=50, top_p=0.9, eos_token_id=-1, max_new_tokens=5, **kw).cpu().tolist()
    return toks, min(margin)


def test_generate_batch_of_two_equals_each_sequence_alone(lm, ops, monkeypatch):
    """B = 2 with left padding and seed=[a, b] == each sequence alone with its seed.  The batch's logits differ from a single sequence's in their last
    bits (other launch shapes), which can move a draw only if its u sits on a boundary of the cumulative distribution: a and b are the first seeds of
    a fixed list for which every draw of the single-sequence run lies more than 1e-4 from every boundary (asserted), fp32 logit noise being ~1e-6."""
    from tests import util as U
    g = U.gold("llm_tiny")
    emb = torch.from_numpy(g["emb"][:, :40].copy()).to(DEV)
    mask = torch.ones((2, 40), dtype=torch.long, device=DEV)
    mask[1, :7] = 0
    chosen, alone = [], []
    for b, cands in enumerate(([11, 12, 13, 14, 15, 16], [29, 30, 31, 32, 33, 34])):
        for s in cands:
            toks, margin = _recorded(lm, ops, monkeypatch, s, inputs_embeds=emb[b:b + 1], attention_mask=mask[b:b + 1])
            if margin > 1e-4:
                chosen.append(s); alone.append(toks[0])
                break
    assert len(chosen) == 2, "no seed of the list keeps every draw 1e-4 away from the CDF boundaries"
    both, margin = _recorded(lm, ops, monkeypatch, chosen, inputs_embeds=emb, attention_mask=mask)
    assert margin > 5e-5
    assert both == alone


def test_generate_seeded_stop_is_pipelined_and_exact(lm):
    """A token of the seeded run as eos: the result is the run's prefix up to and including its first occurrence, whether the stop test looks every
    step or eight steps late (the surplus steps draw from (seed, step) and change nothing), and the same seed afterwards still gives the full run."""
    full = _gen(lm, 21, n=8, top_p=0.9)[0]
    eos = full[2]
    cut = full[:full.index(eos) + 1]
    for every in (1, 8):
        assert _gen(lm, 21, n=8, top_p=0.9, eos_token_id=eos, eos_check_every=every)[0] == cut
    assert _gen(lm, 21, n=8, top_p=0.9)[0] == full


def test_generate_seed_needs_a_top_k_the_kernel_takes(lm):
    for k in (None, 2000, 0):
        with pytest.raises(ValueError, match="1024"):
            _gen(lm, 5, top_k=k)


def test_generate_without_seed_keeps_the_torch_route(lm, ops, monkeypatch):
    from ullsam_amd.modeling import modeling_internlm2 as M
    calls = []
    real = M._sample

    def fused(*a, **k):
        raise AssertionError("ops.sample_topk_topp called without a seed")

    monkeypatch.setattr(ops, "sample_topk_topp", fused)
    monkeypatch.setattr(M, "_sample", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    t = torch.tensor(IDS, device=DEV)
    torch.manual_seed(0)
    out = lm.generate(input_ids=t, max_new_tokens=3, eos_token_id=-1, do_sample=True, top_k=50, temperature=0.7, top_p=0.9)
    assert out.shape == (1, 8) and len(calls) == 3
