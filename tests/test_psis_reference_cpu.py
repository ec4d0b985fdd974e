"""CPU pins of the PSIS edge suite (tests/psis_reference.py): every boundary number of the launcher, the candidate hand-over design,
the long-double restatement against the CPU oracle on every case, the input condition of the GPU tests (the fp64 oracle itself holds
every case to a tenth of the parity margins) and the detectability of a selection mistake on every tie case."""
import numpy as np
import pytest

from oracle import pf_oracle as po
import margins as mg
import psis_reference as pr

needs_ld = pytest.mark.skipif(not pr.HAVE_LONGDOUBLE, reason=pr.SKIP_REASON)
CASE_IDS = [c.id for c in pr.CASES]


# ---- launch rules ------------------------------------------------------------------------------------------------------------------
def test_tail_length_and_route_boundaries():
    for S in list(range(1, 300)) + [8191, 8192, 64000, 300000, 1863225, 1863226, 2200000]:
        assert pr.tail_length(S) == po.lib().pfo_psis_tail_length(S)
    assert (pr.tail_length(20), pr.tail_length(21)) == (4, 5)
    assert (pr.tail_length(21) + 2) // 4 - 1 == 0                      # xstar slot of the first fit
    assert (pr.route(20), pr.route(21)) == ("single", "single")
    assert pr.route(20, "big") == "single" and pr.route(21, "big") == "big"        # no fit: nothing to sort
    assert (pr.route(8191), pr.route(8192)) == ("single", "multi")
    assert pr.route(8192, "single") == "single" and pr.route(8192, "big") == "big"
    assert (pr.tail_length(1863225) + 1, pr.tail_length(1863226) + 1) == (4096, 4097)
    assert (pr.route(1863225), pr.route(1863226)) == ("multi", "big")
    assert pr.route(1863225, "single") == "single" and pr.route(1863226, "single") == "big"
    assert pr.tail_length(64000) + 1 == 760


def test_key_of_is_the_isless_order():
    nan_p, nan_n = pr._nan(False), pr._nan(True)
    xs = np.array([-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300, np.inf, nan_p])
    k = pr.key_of(xs)
    assert np.all(np.diff(k.astype(object)) > 0)                        # strictly increasing, -0.0 below +0.0, NaN above +Inf
    assert pr.key_of(np.array([nan_n]))[0] == pr.key_of(np.array([nan_p]))[0] == pr.KEY_NAN
    payload = np.array([0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)
    assert np.all(pr.key_of(payload) == pr.KEY_NAN)
    assert pr.KEY_NAN < np.uint64(0xFFFFFFFFFFFFFFFF)                    # the sort's padding sentinel stays last


def test_case_table_sits_on_its_boundaries():
    """every row is where its description says: sizes, routes, shift0, bins, counts of non-finite entries"""
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    for c in pr.CASES:
        S = len(c.lr())
        assert S <= 300000 or c.id.startswith("tailcap_")
        assert set(c.routes) <= set(pr.ROUTES) and "natural" in c.routes
    L = {c.id: c.lr() for c in pr.CASES}
    assert [len(L[i]) for i in ("s20_m4", "s21_m5", "s8191", "s8192", "tailcap_4096", "tailcap_4097")] == \
        [20, 21, 8191, 8192, 1863225, 1863226]
    # key ranges
    assert pr.shift0(L["lowbits"]) == 0 and len(np.unique(pr.key_of(L["lowbits"]) >> np.uint64(11))) == 1
    assert pr.route(len(L["lowbits"])) == "multi" and pr.compact_accepts(L["lowbits"])[1]   # bins are the low 12 key bits
    assert pr.shift0(L["straddle_zero"]) == 52 and L["straddle_zero"].min() < 0 < L["straddle_zero"].max()
    # non-finite rows
    for S in (1000, 8192):
        lr = L[f"neginf_cutoff_{S}"]
        tail, cut = pr.tail_indices(lr)
        assert lr[cut] == -np.inf and np.all(np.isfinite(lr[tail])) and np.sum(np.isinf(lr)) == S - pr.tail_length(S)
    tail, cut = pr.tail_indices(L["neginf_in_tail_8192"])
    assert np.sum(np.isinf(L["neginf_in_tail_8192"][tail])) == 1
    for i in pr.NAN_CASES:
        assert np.sum(np.isnan(L[i])) == 1 and np.signbit(L[i][np.isnan(L[i])][0]) == ("neg" in i)
    assert np.isnan(L["nan_neg_first_64000"][0])
    # degenerate tails: the M + 1 largest are one value
    for i in ("degenerate_1000", "degenerate_8192"):
        tail, cut = pr.tail_indices(L[i])
        assert np.all(L[i][tail] == L[i][cut])
    # tie rows: the cutoff is tied with the tail, and the tied indices differ where the row says
    for c in pr.CASES:
        if c.tie:
            tail, cut = pr.tail_indices(c.lr())
            assert pr.key_of(c.lr())[tail[0]] == pr.key_of(c.lr())[cut], c.id
    for i, byte in (("ties_byte1", 1), ("ties_byte2", 2)):
        lr = L[i]
        tail, cut = pr.tail_indices(lr)
        grp = np.flatnonzero(lr == lr[cut])
        assert len(grp) >= 5 and len(set((grp & ~(0xFF << (8 * byte))).tolist())) == 1 and len(set(grp.tolist())) == len(grp)
        assert 0 < np.sum(np.isin(grp, tail)) < len(grp)
    assert pr.route(len(L["ties_round_30000"])) == "multi" and not pr.compact_accepts(L["ties_round_30000"])[1]


@pytest.mark.parametrize("ntop,accepted", [(760, True), (761, True), (4096, True), (4097, False)])
def test_compact_design_counts(ntop, accepted):
    """the threshold bin (sign + exponent of [8, 16) = 3074) and above hold exactly ntop elements; R = 760; <= 4096 is handed over"""
    lr = pr.case_lr(f"compact_{ntop}")
    assert len(lr) == 64000 and pr.tail_length(64000) + 1 == 760 and pr.shift0(lr) == 52
    count, ok, b = pr.compact_accepts(lr)
    assert (count, ok, b) == (ntop, accepted, 3074)
    assert np.sum(pr.bin_of(lr) >= 3074) == ntop and np.sum(pr.bin_of(lr) > 3074) == 0


# ---- selection: the oracle's comparator is the (isless, index) order ---------------------------------------------------------------
def _smoothed(lr, lw):
    """indices whose log weight is not lr - const, i.e. the entries PSIS replaced"""
    fin = np.isfinite(lr) & np.isfinite(lw)
    d = lw[fin] - lr[fin]
    const = np.median(d)                                               # the tail is at most a fifth of the pool
    return set(np.flatnonzero(fin)[np.abs(d - const) > 1e-9 * (1 + abs(const))].tolist())


@pytest.mark.parametrize("id", [c.id for c in pr.CASES if c.tie])
def test_oracle_selects_the_isless_index_tail(id):
    lr = pr.case_lr(id)
    lw, w, k, M = pr.case_oracle(id)
    tail, cut = pr.tail_indices(lr)
    assert np.isfinite(k)
    sm = _smoothed(lr, lw)
    assert sm <= set(tail.tolist()) and cut not in sm
    tied_in = [int(i) for i in tail if pr.key_of(lr)[i] == pr.key_of(lr)[cut]]
    assert set(tied_in) <= sm, "a tied tail entry kept its raw weight"


# ---- the long-double restatement, the condition of every case and the detectability of every tie case ------------------------------
def _devs(lw, w, k, lw_o, w_o, k_o):
    fin = np.isfinite(lw_o)
    d = {"psis_logw": 0.0, "psis_w": 0.0, "pareto_k": 0.0}
    if fin.any():
        d["psis_logw"] = float(np.max(np.abs(lw[fin] - lw_o[fin]) / (1 + np.abs(lw_o[fin]))))
    wf = np.isfinite(w_o)
    if wf.any() and np.max(w_o[wf]) > 0:
        d["psis_w"] = float(np.max(np.abs(w[wf] - w_o[wf])) / np.max(w_o[wf]))
    if np.isfinite(k_o):
        d["pareto_k"] = float(abs(k - k_o))
    return d


@needs_ld
@pytest.mark.parametrize("id", CASE_IDS)
def test_oracle_holds_every_case_to_a_tenth_of_the_margins(id):
    """oracle (fp64) minus long double, per case: same finite / NaN pattern, and every deviation under margin / 10 -- the condition
    for using the oracle as the GPU tests' reference at the full margin.  Measured worst over this table (x86-64 long double):
    psis_logw 5.8e-15, psis_w 6.3e-14, pareto_k 2.1e-14, all three on tailcap_4097 (margin / 10: 1e-11, 1e-11, 1e-9)."""
    lr = pr.case_lr(id)
    lw_o, w_o, k_o, M = pr.case_oracle(id)
    tail, cut = pr.tail_indices(lr)
    assert M == pr.tail_length(len(lr))
    lw, w, k = pr.psis_longdouble(lr, tail, cut)
    np.testing.assert_array_equal(np.isnan(lw_o), np.isnan(lw.astype(np.float64)))
    np.testing.assert_array_equal(np.isfinite(lw_o), np.isfinite(lw.astype(np.float64)))
    np.testing.assert_array_equal(np.isnan(w_o), np.isnan(w.astype(np.float64)))
    assert np.isnan(k_o) == bool(np.isnan(k))
    d = _devs(lw, w, k, lw_o.astype(pr.LD), w_o.astype(pr.LD), pr.LD(k_o))
    print(f"condition {id}: " + " ".join(f"{q} {v:.3g}" for q, v in d.items()) + f" k {k_o:.4f}")
    for q, v in d.items():
        assert v <= 0.1 * mg.CONTRACT[q], (id, q, v)
    if np.isfinite(np.sum(w_o)):
        assert abs(float(np.sum(w)) - 1.0) <= 1e-15 * 10 and abs(np.sum(w_o) - 1.0) <= 1e-12


@needs_ld
@pytest.mark.parametrize("id", [c.id for c in pr.CASES if c.tie])
def test_a_tie_on_the_wrong_side_is_visible(id):
    """exchanging the tied entry just inside the tail with the tied cutoff entry moves their log weights by >= 1e4 margins: a kernel
    that breaks the tie the other way cannot pass the psis_logw check of this row"""
    lr = pr.case_lr(id)
    tail, cut = pr.tail_indices(lr)
    wrong, cut_w, i_in, i_out = pr.wrong_side(lr)
    assert sorted(set(wrong.tolist()) ^ set(tail.tolist())) == sorted([i_in, i_out])
    lw, _, k = pr.psis_longdouble(lr, tail, cut)
    lw2, _, k2 = pr.psis_longdouble(lr, wrong, cut_w)
    assert k == k2                                                     # the same values are fitted: only the assignment moves
    for i in (i_in, i_out):
        move = float(abs(lw[i] - lw2[i]) / (1 + abs(lw[i])))
        print(f"detectability {id}: index {i} moves {move:.3g}")
        assert move >= 1e4 * mg.CONTRACT["psis_logw"], (id, i, move)


# ---- sampler helpers ---------------------------------------------------------------------------------------------------------------
def test_cdf_hit_uniforms_land_on_a_cdf_entry():
    """the uniforms handed to the GPU sampler as "exactly on a CDF entry" are that, and the oracle then takes the next positive index"""
    for S in (4096, 4097, 65537):                                      # (about one CDF entry in 512 can be hit by a 53-bit uniform)
        _, w, _, _ = po.psis(pr.sampler_log_ratios(S, S))
        assert w[0] == 0.0 and w[-1] == 0.0 and np.sum(w == 0.0) > S // 10
        u = pr.cdf_hit_uniforms(w)
        assert len(u) > 0
        C = pr.fixed_cdf(w)
        idx = po.sample_weighted(w, len(u), uniforms=u)
        for ui, i in zip(u, idx):
            r = ((int(ui * 9007199254740992.0) << 11) * C[-1]) >> 64
            assert r in C and C[i] > r and (i == 0 or C[i - 1] == r) and w[i] > 0
    _, w, _, _ = po.psis(pr.sampler_log_ratios(300, 1, one_hot=True))
    assert np.sum(w == 1.0) == 1 and np.sum(w == 0.0) == 299
