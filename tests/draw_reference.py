"""Extended-precision per-coordinate reference of the three kernels that write draws, and a Python mirror of their dispatch.  Not
collected by pytest; used by tests/test_gpu_draw_reference.py and pinned on the CPU by tests/test_draw_reference_cpu.py.  Built on
tests/scan_reference.py (normals, LDFactor, target_logp).

  pf_elbo_xw_kernel<KC>                       the streaming writer          (pathfinder.jl_amd/csrc/elbo_xw_kernel.hip)
  pf_elbo_mfma_kernel<KC, NBW, TGT, RPAD, WX> the two-pass MFMA kernel      (pathfinder.jl_amd/csrc/elbo_mfma_kernel.hip)
  pf_elbo_draws_kernel<KPAD, TGT, RPAD, MEM>  the lane-per-draw kernel      (pathfinder.jl_amd/csrc/elbo_kernels.hip)

All three perform the same operation on one fit (s = sqrt(alpha), Householder vectors Vh (d x k, unit diagonal), the compact-WY
T (k x k upper), the Cholesky factor V (k x k upper), mu; k = min(d, 2 j)) and normals u:
    z = [V' u_1; u_2],   w = Vh' z,   tv = T w,   x = mu + s . (z - Vh tv)
DrawRef computes, in np.longdouble, for a set of draw indices of ONE fit whose arrays are the GPU's own (eng.get_fit):
  X_wy    the statement above with the GPU's downloaded T.  THIS is what is asserted: it isolates the draw kernel from the rounding
          the fit kernel left in T (T is an input of the draw kernels, like Vh and V).
  X_refl  the reflector-by-reflector form x = mu + s . H_0 .. H_{k-1} z of LDFactor.draws (tau = diag T): recorded, never asserted --
          |X_wy - X_refl| is the fit kernel's rounding in the off-diagonal of T, seen through the draws.
  S_x     the per-coordinate scale S_x[i, n] = |mu_i| + s_i Ya[i, n],  Ya = |z| + |Vh| |T| |Vh|' |z|,  |z| = [|V|' |u_1|; |u_2|]:
          the same sums with every term replaced by its absolute value (the GPU's |T|, not the reference's |Tw|).  A rounding error
          of relative size eps in any term of the kernels' sums moves x[i, n] by at most eps S_x[i, n].
  lq, lp, S_q, S_p  as scan_reference.Ref computes them (lp and S_p from X_wy and this Ya).

Tolerances (derived here, never fitted to what the GPU returns; eps = 2^-52, i.e. TWO unit roundoffs per counted step):
  |x - X_wy| <= C_x eps S_x,   C_x = L_w + 3 KC + 16
      L_w    length of the accumulation chain of w = Vh'z, the only chain that grows with d:
             lane    L_w = d              w[j] += Vh[i][j] z[i] row after row, one fma per row (elbo_kernels.hip, the head rows then pass 1)
             writer  L_w = 4 nblk         per 16-row block four v_mfma_f64_4x4x4 on the same accumulator (r = 0 .. 3, each contracting the
                                          4 rows 4 q + r, q = 0 .. 3); a wave owns its 16 draws end to end, so nothing is summed across waves
                                          and the chunks of a streamed factor continue the same accumulators (elbo_xw_kernel.hip body1)
             two-pass L_w = 4 NBW + 8     a wave accumulates its NBW blocks (4 MFMAs each), then the 8 per-wave partial tiles are summed
                                          through LDS (elbo_mfma_kernel.hip `red` -> `wsum`)
      3 KC   the head transform V'u_1, tv = T w and Vh[i, :] tv: three contractions of at most KC terms
      16     the roundings of the inputs (u, s, mu as double), the final multiply-add, and slack for the order of the last adds
  |lq - lq_ref| <= C_q eps S_q,  C_q = 4 nblk + 16 (the scan's, shared by writer and two-pass kernel: the same lane ownership);
                                 lane: d + 16 (|u|^2 one fma per row)
  |lp - lp_ref| <= C_p eps S_p,  C_p = 8 nblk + 4 KC + 32 (the scan's; two-pass kernel and writer-then-scan);
                                 lane: 2 d + 4 KPAD + 32 (x's own chain and the target's row sums, each d long)
      the lane and two-pass kernels evaluate the target directly from x; S_p is built from |x - m| <= |mu - m| + s Ya and
      dominates every term of that direct form.
"""
import numpy as np

import scan_reference as sr
from helpers import oracle_factor_from_gpu

LD = sr.LD
EPS = sr.EPS64
EPSLD = float(np.finfo(LD).eps)

XW_KCS = (4, 8, 12, 16, 20, 32)
MF_KCS = (4, 8, 12, 16)
LANE_KPADS = (4, 8, 12, 16, 20, 32, 64)
FAMILIES = ((0, 0), (2, 0), (1, 0), (1, 8), (1, 16))          # (TGT, RPAD): none, funnel, Gaussian rank padding 0 / 8 / 16
LDS_LIMIT = 160 * 1024
ICDF_B = sr._tab_const("PF_ICDF_B")


def kpad_for(J):
    return next(o for o in LANE_KPADS if 2 * J <= o)


# ---- tolerances ----------------------------------------------------------------------------------------------------------------
def nblk_of(d):
    return (d + 15) // 16


def nbw_of(d):
    n = (nblk_of(d) + 7) // 8
    return 1 if n <= 1 else 2 if n <= 2 else 4 if n <= 4 else 8


def c_x(kern, d, kc):
    L = {"lane": d, "xw": 4 * nblk_of(d), "mf": 4 * nbw_of(d) + 8}[kern]
    return L + 3 * kc + 16


def c_q(kern, d):
    return d + 16 if kern == "lane" else 4 * nblk_of(d) + 16


def c_p(kern, d, kc):
    return 2 * d + 4 * kc + 32 if kern == "lane" else 8 * nblk_of(d) + 4 * kc + 32


# ---- the reference -------------------------------------------------------------------------------------------------------------
def wy_draws(L, T, U):
    """(X_wy, Ya) in long double: compact WY with the given T (k x k, upper triangle read), L an LDFactor, U (d, n) normals"""
    k = L.k
    Z = np.asarray(U, dtype=LD).copy()
    Za = np.abs(Z)
    if not k:
        return L.mu[:, None] + L.s[:, None] * Z, Za
    T = np.triu(np.asarray(T, dtype=LD)[:k, :k])
    Z[:k] = L.V.T @ Z[:k]
    Za[:k] = np.abs(L.V).T @ Za[:k]
    tv = T @ (L.Vh.T @ Z)
    X = L.mu[:, None] + L.s[:, None] * (Z - L.Vh @ tv)
    Ya = Za + np.abs(L.Vh) @ (np.abs(T) @ (np.abs(L.Vh).T @ Za))
    return X, Ya


class DrawRef:
    """long-double reference of draws n0 + idx (or of the host normals U) of one fit `f` (a pfmi_get_fit dictionary), target tg or None"""

    def __init__(self, f, tg, seed, idx, n0=0, U=None):
        F = oracle_factor_from_gpu(f)
        L = sr.LDFactor(F, f["mu"])
        d = L.d
        self.idx = np.asarray(idx, dtype=np.int64)
        U = sr.normals(seed, d, n0, self.idx) if U is None else np.asarray(U, dtype=np.float64)[:, self.idx]
        self.U, self.L = U, L
        self.X_wy, Ya = wy_draws(L, f["T"], U)
        self.X_refl, _ = L.draws(U)
        self.S_x = (np.abs(L.mu)[:, None] + L.s[:, None] * Ya).astype(np.float64)
        self.X = self.X_wy.astype(np.float64)
        usq = np.sum(np.asarray(U, dtype=LD) ** 2, axis=0)
        self.lq = (-(d * sr.LOG2PI + L.logdet + usq) / 2).astype(np.float64)
        self.S_q = ((d * sr.LOG2PI + abs(L.logdet) + usq) / 2).astype(np.float64)
        self._Ya = Ya
        self.lp = self.S_p = None
        if tg is not None:
            self.lp, self.S_p = self.target(tg)

    def target(self, tg):
        """(lp, S_p) of the same draws under another target"""
        L = self.L
        Ea = np.abs(L.mu - np.asarray(tg.mean, dtype=LD) if tg.kind != 1 else L.mu)[:, None] + L.s[:, None] * self._Ya
        lp, Sp = sr.target_logp(tg, self.X_wy, Ea)
        return lp.astype(np.float64), Sp.astype(np.float64)

    def x_ratio(self, X):
        """|X - X_wy| / (eps S_x), (d, n): X the GPU's columns of self.idx"""
        dev = np.abs(np.asarray(X, dtype=LD) - self.X_wy).astype(np.float64)
        return dev / (EPS * self.S_x)

    def refl_ratio(self):
        return np.abs(self.X_wy - self.X_refl).astype(np.float64) / (EPS * self.S_x)

    def col_rel(self, X):
        """the contract's unit: |dx| / (1 + max_i |x|) per column"""
        return np.abs(X - self.X) / (1 + np.abs(self.X).max(axis=0))


# ---- a plain float64 statement of the lane kernel, with the mutations the checker must catch --------------------------------------
MUTATIONS = ("t_offdiag_zero", "t_transposed", "head_omitted", "head_pad_rows", "neighbour_counter", "sqrt_alpha_swapped",
             "w_last_block", "w_last_chunk", "mu_last_dropped")


def lane_f64(f, U, kc, mut=None, ch_rows=256, U_next=None):
    """x (d, n) in float64, compact WY in the lane kernel's order (row after row, columns padded to kc with an identity-padded V).
    `mut`: one of MUTATIONS -- a wrong kernel.  ch_rows: rows per streamed chunk (w_last_chunk); U_next: the normals of the draws with
    the next counter (neighbour_counter)."""
    d = len(f["alpha"])
    k = min(d, f["qr_factors"].shape[1])
    s, mu = np.sqrt(f["alpha"]), np.array(f["mu"], dtype=np.float64)
    Vh = np.zeros((d, kc))
    for c in range(k):
        Vh[c, c] = 1.0
        Vh[c + 1:, c] = f["qr_factors"][c + 1:, c]
    T = np.zeros((kc, kc))
    T[:k, :k] = np.triu(f["T"])
    V = np.eye(kc)
    V[:k, :k] = np.triu(f["V"])
    U = np.array(U, dtype=np.float64)
    if mut == "neighbour_counter":
        U[d // 2] = U_next[d // 2]
    if mut == "t_offdiag_zero":
        a, b = np.unravel_index(np.argmax(np.abs(np.triu(T, 1))), T.shape)
        assert T[a, b] != 0
        T[a, b] = 0.0
    if mut == "t_transposed":
        T = T.T.copy()
    if mut == "sqrt_alpha_swapped":
        i = int(np.argmax(np.abs(np.diff(s))))
        s = s.copy()
        s[[i, i + 1]] = s[[i + 1, i]]
    if mut == "mu_last_dropped":
        mu[d - 1] = 0.0
    if mut == "head_pad_rows":                               # rows k .. min(d, kc) - 1 treated as head rows of a V without its identity padding
        assert k < min(d, kc)
        V[k:, k:] = 0.0
    Z = U.copy()
    h = min(d, kc)
    if mut != "head_omitted":
        Zh = np.zeros((kc, U.shape[1]))
        Zh[:h] = U[:h]
        for a in range(kc - 1, -1, -1):
            acc = np.zeros(U.shape[1])
            for b in range(a + 1):
                acc = acc + V[b, a] * Zh[b]
            Zh[a] = acc
        Z[:h] = Zh[:h]
    rows = d
    if mut == "w_last_block":
        rows = (nblk_of(d) - 1) * 16
    if mut == "w_last_chunk":
        rows = ((d - 1) // ch_rows) * ch_rows
        assert 0 < rows < d
    w = np.zeros((kc, U.shape[1]))
    for i in range(rows):
        w = w + Vh[i][:, None] * Z[i][None, :]
    tv = np.zeros_like(w)
    for a in range(kc):
        acc = np.zeros(U.shape[1])
        for b in range(a, kc):
            acc = acc + T[a, b] * w[b]
        tv[a] = acc
    X = np.empty_like(U)
    for i in range(d):
        v = Z[i].copy()
        for j in range(kc):
            v = v - Vh[i, j] * tv[j]
        X[i] = mu[i] + s[i] * v
    return X


# ---- Python mirror of the dispatch (pf_launch_elbo_draws, launch_mf_k / launch_mf, launch_xw with xw_lds_bytes) ---------------------
def xw_lds_bytes(ch_blocks, nchunks, kc):
    stage = (ch_blocks * 16 * kc + ch_blocks * 32) * (2 if nchunks > 1 else 1)
    stage = max(stage, 1024)                                                      # XW_MIN_FRONT
    return 8 * (stage + kc * kc + 4 * (sr.ICDF_NB_LDS << ICDF_B))


def xw_chunking(d, kc):
    """(ch_blocks, nchunks) of launch_xw: resident when the whole block fits 160 KB, else chunks of 16 blocks (8 at KC = 32)"""
    nblk = nblk_of(d)
    if xw_lds_bytes(nblk, 1, kc) > LDS_LIMIT:
        chb = 8 if kc > 20 else 16
        return chb, (nblk + chb - 1) // chb
    return nblk, 1


def xw_max_resident_d(kc):
    d = 16
    while xw_chunking(d + 16, kc)[1] == 1:
        d += 16
    return d


def mf_lds_bytes(d, kc, rpad):
    rows = nblk_of(d) * 16
    q = (rpad + 3) // 4
    return 8 * (rows * kc + 3 * rows + kc * kc + 8 * 64 * (kc // 4) + 8 * 64 * q + 256 + 64 * q + 32 + rpad * rpad + 8 * 64
                + 4 * (12 << ICDF_B) + 2)


def mf_handles(d, kc, tgt, rpad):
    return kc in MF_KCS and d <= 1024 and mf_lds_bytes(d, kc, rpad if tgt == 1 else 0) <= LDS_LIMIT


def mf_max_d(kc, tgt, rpad):
    return max(d for d in range(1, 1025) if mf_handles(d, kc, tgt, rpad))


def plan_for(d, kc, tgt, rpad, N, nfits, x, mem=False, force=None, ncu=256):
    """the draw-kernel plan ONE pf_launch_elbo_draws call takes (None: the call is a scan's, no draw kernel runs): kc = the fit's
    column padding, (tgt, rpad) the target family the call passes, x = draws written, mem = host normals, force = PFMI_ELBO_KERNEL"""
    f = force[0] if force else ""
    if not mem and f != "l":
        mf_shape = d <= 1024 and kc <= 16
        want_qf = f == "q" or (f != "m" and (N >= 64 or (not mf_shape and N >= 16)))
        if want_qf and not x and kc <= 32:
            return None
        want_xw = x and (f == "x" or (f != "m" and not (tgt != 0 and mf_shape)))
        ngroups = (N + 15) // 16
        if want_xw and kc in XW_KCS:
            chb, nch = xw_chunking(d, kc)
            split, min_piece = 1, (4 if nch > 1 else 16)
            while split * nfits < 2 * ncu and ngroups // (split * 2) >= min_piece:
                split *= 2
            return f"xw:{kc}:{'stream' if nch > 1 else 'res'}:{'split' if split > 1 else 'whole'}"
        if mf_handles(d, kc, tgt, rpad):
            split = 1
            while split * nfits < ncu and split * 2 <= ngroups:
                split *= 2
            return f"mf:{kc},{nbw_of(d)},{tgt},{rpad}:{'x' if x else 'nox'}:{'split' if split > 1 else 'whole'}"
    return f"lane:{kc},{tgt},{rpad}:{'u' if mem else 'rng'}:{'x' if x else 'nox'}"


ALL_PLANS = ([f"xw:{kc}:{st}:{cut}" for kc in XW_KCS for st in ("res", "stream") for cut in ("whole", "split")]
             + [f"mf:{kc},{nbw},{t},{r}:{wx}:{cut}" for kc in MF_KCS for nbw in (1, 2, 4, 8) for t, r in FAMILIES for wx in ("x", "nox")
                for cut in ("whole", "split")]
             + [f"lane:{kp},{t},{r}:{m}:{wx}" for kp in LANE_KPADS for t, r in FAMILIES for m in ("u", "rng") for wx in ("x", "nox")])

EXCLUDED = {
    "mf:<KC>,<NBW>,0,0:nox:<cut>": "no target and no draws: every call site without a built-in target (host / device closures, pool, "
                                   "pfmi_draws) passes a buffer for x, so the two-pass kernel never runs <TGT = 0, WX = false>",
    "lane:<KPAD>,0,0:<u|rng>:nox": "the same call sites: a launch without a built-in target always writes its draws",
}


def excluded(name):
    """the reason a plan cannot be reached through the API, or None"""
    if name.startswith("mf:") and ",0,0:nox:" in name:
        return EXCLUDED["mf:<KC>,<NBW>,0,0:nox:<cut>"]
    if name.startswith("lane:") and ",0,0:" in name and name.endswith(":nox"):
        return EXCLUDED["lane:<KPAD>,0,0:<u|rng>:nox"]
    if name.startswith("mf:"):
        kc, nbw, t, r = (int(v) for v in name.split(":")[1].split(","))
        lo = {1: 1, 2: 129, 4: 257, 8: 513}[nbw]
        if not mf_handles(lo, kc, t, r):
            return f"the factor block of the smallest d with NBW = {nbw} (d = {lo}) needs more than 160 KB of LDS at KC = {kc}, RPAD = {r}"
    return None


REACHABLE = [nm for nm in ALL_PLANS if excluded(nm) is None]


# ---- the grid: setups (one fit_batch each) and the draw calls made on them -----------------------------------------------------------
# tests/test_gpu_draw_reference.py runs every call and asserts call_plan(); tests/test_draw_reference_cpu.py proves that the calls'
# plans are exactly REACHABLE.
import collections

Fit = collections.namedtuple("Fit", "d J K L")                # K synthetic paths of L + 1 points fitted with history length J
Call = collections.namedtuple("Call", "route tgt rpad N force mem n0", defaults=(None, False, 0))
# route: "draws" (pfmi_draws: one fit, x), "pool" (pfmi_pool_build: K fits, x), "batch" (pfmi_elbo_batch: K L fits, no x)
J_OF_KC = {4: 2, 8: 4, 12: 6, 16: 8, 20: 10, 32: 16, 64: 17}


def call_plan(fit, c, ncu=256):
    nfits = {"draws": 1, "pool": fit.K, "batch": fit.K * fit.L}[c.route]
    return plan_for(fit.d, kpad_for(fit.J), c.tgt, c.rpad, c.N, nfits, c.route != "batch", c.mem, c.force, ncu)


def _xw_force(fit, c):
    """the call with PFMI_ELBO_KERNEL=xw where the default route would not be the writer"""
    return c if (call_plan(fit, c) or "").startswith("xw:") else c._replace(force="xw")


def _mf_force(fit, c):
    return c if (call_plan(fit, c) or "").startswith("mf:") else c._replace(force="mfma")


def writer_matrix():
    """every KC at the largest resident and the smallest streamed d, + KC = 32 at d = 512 / 513 and KC = 12 at d = 1281 / 1536"""
    out = []
    for kc in XW_KCS:
        J, dres = J_OF_KC[kc], xw_max_resident_d(kc)
        for d in [dres, dres + 1] + {32: [512, 513], 12: [1281, 1536]}.get(kc, []):
            fit = Fit(d, J, 1, J + 2)
            calls = [Call("draws", 0, 0, 100), _xw_force(fit, Call("draws", 1, 0, 100)), Call("draws", 0, 0, 512)]
            out.append((fit, calls))
    return out


def writer_d_edges():
    out = []
    for kc, ds in ((12, (1, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 65)), (20, (1, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 65)), (32, (31, 33))):
        for d in ds:
            fit = Fit(d, J_OF_KC[kc], 1, J_OF_KC[kc] + 2)
            out.append((fit, [Call("draws", 0, 0, 100), _xw_force(fit, Call("draws", 1, 0, 100))]))
    return out


WRITER_N = (1, 15, 16, 17, 255, 256, 257, 512, 1000)
WRITER_N0 = (0, 53, 2 ** 32 - 5)


def writer_n_edges():
    out = []
    for kc in (8, 20):
        fit = Fit(70, J_OF_KC[kc], 1, J_OF_KC[kc] + 2)
        out.append((fit, [Call("draws", 0, 0, N, n0=n0) for N in WRITER_N for n0 in WRITER_N0]))
    return out


def mf_d_list(kc):
    d8 = min(mf_max_d(kc, t, r) for t, r in FAMILIES)
    return [113, 250, 500, 1000] + ([d8] if 513 <= d8 < 1000 else [])


def mf_matrix():
    """every (KC, NBW) x the five families x {x, nox} x {whole, split}: x through pfmi_draws at N = 100 (split) and N = 16 (whole),
    nox through pfmi_elbo_batch at N = 48 (split) and N = 5 (whole).  Where the factor block does not fit the two-pass kernel's LDS
    (KC = 12 / 16 at d = 1000) the call falls through to the lane kernel -- call_plan says so -- and the largest d at which every
    family fits is added."""
    out = []
    for kc in MF_KCS:
        for d in mf_d_list(kc):
            fit = Fit(d, J_OF_KC[kc], 2, J_OF_KC[kc] + 1)
            calls = []
            for t, r in FAMILIES:
                calls += [_mf_force(fit, Call("draws", t, r, 100)), _mf_force(fit, Call("draws", t, r, 16))]
                if t:
                    calls += [Call("batch", t, r, 48), Call("batch", t, r, 5)]
            out.append((fit, calls))
    return out


def mf_edges():
    """NBW boundaries d = 128 / 129, 256 / 257, 512 / 513, 1024 at KC = 8, N in {5, 16, 17, 48}, rank-8 Gaussian"""
    out = []
    for d in (128, 129, 256, 257, 512, 513, 1024):
        fit = Fit(d, 4, 2, 5)
        out.append((fit, [Call("draws", 1, 8, N) for N in (5, 16, 17, 48)] + [Call("batch", 1, 8, N) for N in (5, 16, 17, 48)]
                    + [Call("pool", 1, 8, 1000)]))
    return out


def lane_matrix():
    """every KPAD x the five families x {host u, generator} x {x, nox} at d = 50; the rank-0 Gaussian again at d = 257 (N = 100) and at
    N = 257 (two blocks of 256 threads)"""
    out = []
    for kp in LANE_KPADS:
        J = J_OF_KC[kp]
        for d in (50, 257):
            fit = Fit(d, J, 1, J + 2)
            calls = []
            for t, r in (FAMILIES if d == 50 else ((1, 0),)):
                for mem in (True, False):
                    force = None if mem else "lane"
                    calls.append(Call("draws", t, r, 100, force, mem))
                    if t:
                        calls.append(Call("batch", t, r, 100, force, mem))
            if d == 50:
                calls += [Call("draws", 1, 0, 257, None, True), Call("draws", 1, 0, 257, "lane", False)]
            out.append((fit, calls))
    return out


def lane_d_edges():
    out = []
    for kp in LANE_KPADS:
        for d in sorted({1, 3, kp - 1, kp, kp + 1}):
            fit = Fit(d, J_OF_KC[kp], 1, J_OF_KC[kp] + 2)
            out.append((fit, [Call("draws", 1, 0, 100, None, True), Call("draws", 1, 0, 100, "lane", False)]))
    return out


GROUPS = {"writer_matrix": writer_matrix, "writer_d_edges": writer_d_edges, "writer_n_edges": writer_n_edges, "mf_matrix": mf_matrix,
          "mf_edges": mf_edges, "lane_matrix": lane_matrix, "lane_d_edges": lane_d_edges}


def grid_plans():
    """{plan name: number of grid calls that take it}"""
    seen = collections.Counter()
    for g in GROUPS.values():
        for fit, calls in g():
            for c in calls:
                seen[call_plan(fit, c)] += 1
    return seen
