"""Reference side of the PSIS / index-selection edge suite (test infrastructure, no GPU).

Four things live here, each stated once and shared by tests/test_psis_reference_cpu.py (which pins them against the CPU oracle) and
tests/test_gpu_psis_edges.py (which runs the kernels on them):

1. The launch rules of csrc/psis_kernels.hip, restated: `tail_length`, `key_of`, `shift0`, `bin_of`, `route`, `compact_accepts`.
   They say which kernel route a pool takes and whether the candidate list of the multi-workgroup route is handed over, so that every
   row of the case table can be pinned to the boundary it is meant to sit on.
2. The selection rule of the reference: PSIS.psis (called at reference src/resample.jl:78) sorts the log ratios with Julia's default
   order, `isless` (-0.0 < +0.0, every NaN greatest), and the sort is stable, i.e. ties go by index.  `tail_indices` is that order.
3. `psis_longdouble`: the tail fit and the normalisation in np.longdouble (Zhang-Stephens grid, posterior-mean theta, prior-adjusted
   k, quantile replacement, clamp at 0, logsumexp), given the selected indices.  It measures how well the fp64 oracle itself holds a
   case: a case enters the GPU suite only when oracle minus long double stays under a tenth of the parity margins.
4. `CASES`: the table of pools (id, generator from a fixed seed, forced routes), and the sizes and weights for the index samplers.
"""
import functools
import math

import numpy as np

LD = np.longdouble
HAVE_LONGDOUBLE = np.finfo(LD).nmant >= 63
SKIP_REASON = "np.longdouble carries fewer than 63 mantissa bits here: no extended-precision reference"

# ---- 1. launch rules (csrc/psis_kernels.hip: pf_launch_psis, pf_key_of, pf_psis_shift0, pf_psis_compact_kernel) ---------------------
TAILCAP = 4096                  # LDS tail capacity: M + 1 <= TAILCAP or the global-sort route
PSIS_MULTI_MIN = 8192           # S >= this: multi-workgroup route
_SIGN = np.uint64(0x8000000000000000)
KEY_NAN = np.uint64(0xFFF8000000000000)
ROUTES = ("natural", "single", "big")   # no forcing, PFMI_PSIS_KERNEL=single, PFMI_PSIS_KERNEL=big


def tail_length(S):
    """M = min(cld(S, 5), ceil(3 sqrt(S)))"""
    return min((S + 4) // 5, int(math.ceil(3.0 * math.sqrt(float(S)))))


def key_of(x):
    """order-preserving map float64 -> uint64 in isless order: -0.0 below +0.0, every NaN one key above +Inf"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = x.view(np.uint64)
    k = np.where((b >> np.uint64(63)) != 0, ~b, b | _SIGN)
    return np.where(np.isnan(x), KEY_NAN, k).astype(np.uint64)


def shift0(lr):
    """right shift that puts the highest differing key bit of the pool at bit 11 of the 4096-bin histogram index (0 when below)"""
    k = key_of(lr)
    diff = int(k.min()) ^ int(k.max())
    top = diff.bit_length() - 1 if diff else 0
    return top - 11 if top >= 11 else 0


def bin_of(lr):
    return ((key_of(lr) >> np.uint64(shift0(lr))) & np.uint64(0xFFF)).astype(np.int64)


def route(S, force=None):
    """"single" | "multi" | "big" for a pool of S log ratios; force: None, "single" or "big" (PFMI_PSIS_KERNEL)"""
    M = tail_length(S)
    if M + 1 > TAILCAP or (force == "big" and M >= 5 and M + 1 <= S):
        return "big"
    if S >= PSIS_MULTI_MIN and M >= 5 and force != "single":
        return "multi"
    return "single"


def compact_accepts(lr):
    """(count, accepted, bin): the population of the threshold bin and everything above it -- the threshold bin is the one the
    (M + 1)-th largest key falls in -- and whether the multi-workgroup route hands that candidate list over (count <= TAILCAP)."""
    R = tail_length(len(lr)) + 1
    hist = np.bincount(bin_of(lr), minlength=4096)
    cum = 0
    for b in range(4095, -1, -1):
        if cum < R <= cum + hist[b]:
            return int(cum + hist[b]), bool(cum + hist[b] <= TAILCAP), b
        cum += int(hist[b])
    return int(cum), False, -1


# ---- 2. selection ------------------------------------------------------------------------------------------------------------------
def tail_indices(lr):
    """(tail, cutoff): the last M indices of the (isless, index) order, ascending, and the index just below them; (None, None)
    where no tail is fitted (M < 5)."""
    S = len(lr)
    M = tail_length(S)
    if M < 5:
        return None, None
    order = np.lexsort((np.arange(S), key_of(lr)))
    return order[S - M:], int(order[S - M - 1])


def wrong_side(lr):
    """The smallest selection mistake at a tie: the tied entry just inside the tail and the tied cutoff entry change places.
    Returns (tail_wrong, cutoff_wrong, i_in, i_out), or None when the cutoff is not tied with the tail."""
    tail, cut = tail_indices(lr)
    k = key_of(lr)
    if k[tail[0]] != k[cut]:
        return None
    wrong = tail.copy()
    i_in = int(tail[0])
    wrong[0] = cut
    return wrong, i_in, i_in, int(cut)                      # the old tail[0] is the new cutoff


# ---- 3. long-double tail fit and normalisation -------------------------------------------------------------------------------------
def _gpd_fit_ld(w):
    """Zhang & Stephens (2009) on ascending w >= 0: (sigma, k) before the prior adjustment (min_points 30, prior 3)"""
    n = len(w)
    m = 30 + int(math.floor(math.sqrt(n)))
    xstar, xmax = w[(n + 2) // 4 - 1], w[n - 1]
    p = (np.arange(1, m + 1, dtype=LD) - LD(0.5)) / LD(m)
    theta = LD(1) / xmax + (LD(1) - np.sqrt(LD(1) / p)) / (LD(3) * xstar)
    kk = np.array([np.sum(np.log1p(-t * w)) / LD(n) for t in theta], dtype=LD)
    ll = LD(n) * (np.log(-theta / kk) - kk - LD(1))
    e = np.exp(ll - np.max(ll))
    th = np.sum(e * theta) / np.sum(e)
    k = np.sum(np.log1p(-th * w)) / LD(n)
    return -k / th, k


def psis_longdouble(lr, tail, cutoff):
    """(log_weights, weights, pareto_k) in np.longdouble for the selection (tail ascending, cutoff); tail None: normalise only.
    The one decision the algorithm takes on fp64 values -- "the shifted tail is identically zero, fit nothing" -- is taken on fp64
    values here too: in long double exp() separates log ratios that fp64 cannot, and the restatement would fit where PSIS does not."""
    lr = np.ascontiguousarray(lr, dtype=np.float64)
    x = lr.astype(LD)
    k = LD(np.nan)
    with np.errstate(all="ignore"):
        if tail is not None and np.all(np.isfinite(lr[tail])):
            M = len(tail)
            lmax, logu = x[tail[-1]], x[cutoff]
            mu = np.exp(logu - lmax)
            w = np.exp(x[tail] - lmax) - mu
            w64 = np.exp(lr[tail] - lr[tail[-1]]) - np.exp(lr[cutoff] - lr[tail[-1]])
            if np.any(w64 != 0.0):
                sigma, k = _gpd_fit_ld(w)
                if np.isfinite(k):
                    k = (k * LD(M) + LD(5)) / (LD(M) + LD(10))
                if np.isfinite(k) and np.isfinite(sigma):
                    p = (np.arange(1, M + 1, dtype=LD) - LD(0.5)) / LD(M)
                    nl = -np.log1p(-p)
                    z = nl if k == 0 else np.expm1(k * nl) / k
                    x[tail] = np.minimum(np.log(sigma * z + mu), LD(0)) + lmax
        if np.any(np.isnan(x)):
            lse = LD(np.nan)
        else:
            mx = np.max(x)
            lse = mx + np.log(np.sum(np.exp(x - mx))) if np.isfinite(mx) else mx
        lw = x - lse
        return lw, np.exp(lw), k


# ---- 4. the case table -------------------------------------------------------------------------------------------------------------
def _nan(negative):
    return np.array([0xFFF8000000000000 if negative else 0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def _light(rng, S):
    """log ratios of a well-behaved pool: k around 0.4-0.5, which the fp64 oracle holds to 1e-12 at every size used here"""
    return rng.normal(size=S) * 1.5 - 3.0


def _g_light(S):
    return lambda rng: _light(rng, S)


def _g_compact(ntop):
    """S = 64 000, R = M + 1 = 760.  Body clip(N(0, 1), +-3.9); `ntop` entries 8 + 8 u^3 share the exponent of [8, 16).  The key range
    spans the sign bit, so shift0 = 52 and a bin is sign plus exponent: the threshold bin (3074) and above hold exactly `ntop`."""
    def g(rng):
        S = 64000
        lr = np.clip(rng.normal(size=S), -3.9, 3.9)
        lr[rng.choice(S, ntop, replace=False)] = 8.0 + 8.0 * rng.random(ntop) ** 3
        return lr
    return g


def _plant_ties(lr, grp, inside, value=None):
    """make lr[grp] one tied value with exactly `inside` of the group in the tail: M - inside of the other entries lie above it"""
    S = len(lr)
    M = tail_length(S)
    others = np.setdiff1d(np.arange(S), grp)
    srt = np.sort(lr[others])
    lo, hi = srt[-(M - inside) - 1], srt[-(M - inside)]
    assert lo < hi
    lr[grp] = 0.5 * (lo + hi) if value is None else value
    return lr


def _g_ties_byte2(rng):
    """S = 300 000: five tied entries at the cutoff whose indices differ only in byte 2 (7 + 65536 j), two of them in the tail"""
    lr = _light(rng, 300000)
    return _plant_ties(lr, 7 + 65536 * np.arange(5), 2)


def _g_ties_byte1(rng):
    """S = 20 000: twelve tied entries at the cutoff whose indices differ only in byte 1 (200 + 256 j), five of them in the tail"""
    lr = _light(rng, 20000)
    return _plant_ties(lr, 200 + 256 * np.arange(12), 5)


def _g_signed_zeros(S):
    """40 log ratios alternating +0.0 / -0.0 straddle the cutoff, 10 of them in the tail: by isless those are the ten +0.0 with the
    largest indices (an order that takes +-0.0 as equal would take the ten largest indices of all forty)."""
    def g(rng):
        M = tail_length(S)
        grp = np.sort(rng.choice(S, 40, replace=False))
        lr = -np.abs(rng.normal(size=S)) * 1.5 - 1e-3
        others = np.setdiff1d(np.arange(S), grp)
        up = rng.choice(others, M - 10, replace=False)
        lr[up] = np.abs(rng.normal(size=M - 10)) * 1.5 + 1e-3
        lr[grp] = np.where(np.arange(40) % 2 == 0, 0.0, -0.0)
        return lr
    return g


def _g_round_ties(S):
    """N(1.3, 0.25) rounded to 0.01: ~50 ties at the cutoff, and the threshold bin [1.5, 2) holds a fifth of the pool, so the candidate
    list of the multi-workgroup route overflows and the tail kernel selects by itself (value and index radix select)"""
    return lambda rng: np.round(1.3 + 0.25 * rng.normal(size=S), 2)


def _g_lowbits(rng):
    """Keys that differ only below bit 11 (shift0 clamps to 0): 2^-20 (1 + j 2^-52), j < 2048.  A spread of 2^-61 is invisible to
    exp() in fp64, so the shifted tail is identically zero and nothing is fitted: the row checks the clamp (bins are then the low 12 key
    bits), the candidate hand-over under it and the normalisation.  (No pool this narrow has a tail fit that fp64 can hold: a relative spread of
    2^-41 is either below the resolution of exp(), or sits on log ratios so large that the logsumexp loses the 1e-10.)"""
    j = rng.integers(0, 2048, size=8192).astype(np.uint64)
    base = np.array([2.0 ** -20]).view(np.uint64)[0]
    return (base + j).view(np.float64)


def _g_neginf(S, n_inf_minus_body):
    """body light, with (S - M) + n_inf_minus_body entries -Inf: 0 puts the cutoff itself at -Inf under an all-finite tail,
    1 puts a -Inf into the tail (no fit)"""
    def g(rng):
        lr = _light(rng, S)
        n = S - tail_length(S) + n_inf_minus_body
        lr[rng.choice(S, n, replace=False)] = -np.inf
        return lr
    return g


def _g_with(S, value, where=None):
    def g(rng):
        lr = _light(rng, S)
        lr[S // 3 if where is None else where] = value
        return lr
    return g


def _g_degenerate(S):
    """the M + 1 largest all equal (400 > M + 1 entries at 5.0 above a clipped body): nz == 0, k NaN, nothing replaced"""
    def g(rng):
        lr = np.minimum(_light(rng, S), 4.0)
        lr[rng.choice(S, 400, replace=False)] = 5.0
        return lr
    return g


class Case:
    def __init__(self, id, gen, routes=ROUTES, seed=0, tie=False, what=""):
        self.id, self.gen, self.routes, self.seed, self.tie, self.what = id, gen, tuple(routes), seed, tie, what

    def lr(self):
        return case_lr(self.id)


_ALL = ROUTES
CASES = [
    # tail-length and route boundaries
    Case("s20_m4", _g_light(20), _ALL, 1, what="M = 4: normalise only on every route"),
    Case("s21_m5", _g_light(21), _ALL, 2, what="M = 5: first fit, xstar slot (M + 2) / 4 - 1 = 0"),
    Case("s8191", _g_light(8191), _ALL, 3, what="last one-workgroup size"),
    Case("s8192", _g_light(8192), _ALL, 4, what="first multi-workgroup size (PSIS_MULTI_MIN)"),
    Case("tailcap_4096", lambda rng: rng.normal(size=1863225), _ALL, 5, what="M + 1 = 4096: LDS tail full, npow = 4096"),
    Case("tailcap_4097", lambda rng: rng.normal(size=1863226), ("natural",), 6, what="M + 1 = 4097: smallest unforced large tail"),
    # candidate hand-over of the multi-workgroup route, R = 760
    Case("compact_760", _g_compact(760), _ALL, 7, what="threshold bin and above hold R: cnt == R"),
    Case("compact_761", _g_compact(761), _ALL, 8, what="cnt == R + 1: the cnt - R + t move skips one"),
    Case("compact_4096", _g_compact(4096), _ALL, 9, what="cnt == TAILCAP: accepted"),
    Case("compact_4097", _g_compact(4097), _ALL, 10, what="cnt == TAILCAP + 1: overflow, the tail kernel selects by itself"),
    # key ranges
    Case("lowbits", _g_lowbits, _ALL, 11, what="keys differ below bit 11: shift0 clamps to 0"),
    Case("straddle_zero", lambda rng: rng.normal(size=20000) * 1.5, _ALL, 12, what="log ratios of both signs: differing bit 63"),
    # ties at the cutoff
    Case("ties_byte1", _g_ties_byte1, _ALL, 13, tie=True, what="tied indices differ in byte 1 only"),
    Case("ties_byte2", _g_ties_byte2, _ALL, 14, tie=True, what="tied indices differ in byte 2 only"),
    Case("ties_round_30000", _g_round_ties(30000), _ALL, 15, tie=True, what="heavy ties, candidate list overflows"),
    Case("signed_zeros_1000", _g_signed_zeros(1000), _ALL, 16, tie=True, what="+-0.0 at the cutoff, one workgroup"),
    Case("signed_zeros_64000", _g_signed_zeros(64000), _ALL, 17, tie=True, what="+-0.0 at the cutoff, multi-workgroup"),
    # non-finite pools
    Case("all_neginf_1000", lambda rng: np.full(1000, -np.inf), _ALL, 18, what="every log ratio -Inf: all NaN"),
    Case("all_neginf_8192", lambda rng: np.full(8192, -np.inf), _ALL, 19, what="the same through the multi-workgroup route"),
    Case("neginf_cutoff_1000", _g_neginf(1000, 0), _ALL, 20, what="S - M entries -Inf: cutoff -Inf, tail finite, mu = 0"),
    Case("neginf_cutoff_8192", _g_neginf(8192, 0), _ALL, 21, what="the same through the multi-workgroup route"),
    Case("neginf_in_tail_8192", _g_neginf(8192, 1), _ALL, 22, what="S - M + 1 entries -Inf: a -Inf in the tail, no fit"),
    Case("neginf_most_8192", _g_neginf(8192, 200), _ALL, 23, what="cutoff and most of the tail -Inf"),
    Case("posinf_8192", _g_with(8192, np.inf), _ALL, 24, what="one +Inf: weights 0 and NaN"),
    Case("nan_pos_1000", _g_with(1000, _nan(False)), _ALL, 25, what="one NaN, sign bit clear"),
    Case("nan_neg_1000", _g_with(1000, _nan(True)), _ALL, 26, what="one NaN, sign bit set (inf - inf on x86)"),
    Case("nan_pos_8192", _g_with(8192, _nan(False)), _ALL, 27, what="one NaN, sign bit clear, multi-workgroup"),
    Case("nan_neg_8192", _g_with(8192, _nan(True)), _ALL, 28, what="one NaN, sign bit set, multi-workgroup"),
    Case("nan_neg_first_64000", _g_with(64000, _nan(True), 0), _ALL, 29, what="negative NaN at index 0"),
    # degenerate tail
    Case("degenerate_1000", _g_degenerate(1000), _ALL, 30, what="M + 1 largest equal, one workgroup"),
    Case("degenerate_8192", _g_degenerate(8192), _ALL, 31, what="M + 1 largest equal, multi-workgroup and large-tail"),
]
CASE = {c.id: c for c in CASES}
NAN_CASES = [c.id for c in CASES if c.id.startswith("nan_")]


@functools.lru_cache(maxsize=None)
def case_lr(id):
    c = CASE[id]
    lr = np.ascontiguousarray(c.gen(np.random.default_rng(1000 + c.seed)), dtype=np.float64)
    lr.setflags(write=False)
    return lr


@functools.lru_cache(maxsize=None)
def case_oracle(id):
    """(log_weights, weights, pareto_k, M) of the CPU oracle, computed once per case and shared (read-only)"""
    from oracle import pf_oracle as po
    lw, w, k, M = po.psis(case_lr(id))
    lw.setflags(write=False)
    w.setflags(write=False)
    return lw, w, k, M


# ---- index samplers ----------------------------------------------------------------------------------------------------------------
CDF_SIZES = (1, 3, 255, 256, 257, 4096, 4097, 65537)       # pf_cdf_kernel: 256-element tiles, 4 per lane, 16 waves
SEQCDF_SIZES = (1, 4095, 4096, 4097, 8193)                 # pf_seqcdf_kernel: 4096-element chunks


def sampler_log_ratios(S, seed, one_hot=False):
    """log ratios whose weights contain exact zeros (-Inf entries), among them both ends of the pool; one_hot: a single weight 1"""
    rng = np.random.default_rng(seed)
    if one_hot:
        lr = np.full(S, -np.inf)
        lr[(2 * S) // 3] = 0.0
        return lr
    lr = rng.normal(size=S) * 1.5
    if S >= 3:
        lr[rng.random(S) < 0.2] = -np.inf
        lr[0] = lr[-1] = -np.inf
        lr[S // 2] = 1.0
    return lr


def fixed_cdf(w):
    """the fixed-point CDF of pf_cdf_kernel as Python integers: prefix sums of floor(w 2^62)"""
    q = [0 if not (x > 0.0) else (1 << 62) if x >= 1.0 else int(math.floor(x * 4611686018427387904.0)) for x in np.asarray(w).tolist()]
    return np.cumsum(np.array(q, dtype=object)).tolist()


def cdf_hit_uniforms(w, limit=16):
    """uniforms u = U 2^-53 whose scaled draw r = floor(U 2^11 Q / 2^64) equals a CDF entry exactly: the draw must then take the NEXT
    positive-weight index (first C[i] > r)"""
    C = fixed_cdf(w)
    Q = C[-1]
    out = []
    for c in sorted(set(C[:-1])):
        if c == 0 or Q == 0:
            continue
        U = -((-c << 53) // Q)                              # ceil(c 2^53 / Q)
        if U < (1 << 53) and ((U << 11) * Q) >> 64 == c:
            out.append(U / 9007199254740992.0)
            if len(out) >= limit:
                break
    return np.array(out, dtype=np.float64)
