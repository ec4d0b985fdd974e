"""CPU side of the uniform mixture of fits (pfmi_mixture_logpdf, MixtureModel): the ABI declarations, the host logic of
MixtureModel against a stand-in engine, and the register / scratch budget of the main mixture kernel."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
from scipy.special import logsumexp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pfmi_mixture_logpdf", "pfmi_mixture_logpdf_dev")


def test_header_symbols_and_library_agree():
    import pfmi
    from pfmi._lib import SYMBOLS
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pfmi.h")).read(), flags=re.S)
    assert re.search(r"int32_t pfmi_mixture_logpdf\(pfmi_ctx \*ctx, int32_t K, const int64_t \*points, int64_t N, const double \*X,"
                     r"\s*double \*lse,\s*double \*comp\);", txt)
    assert re.search(r"int32_t pfmi_mixture_logpdf_dev\(pfmi_ctx \*ctx, int32_t K, const int64_t \*points, int64_t N, const void \*X_dev,"
                     r"\s*void \*lse_dev,\s*void \*comp_dev\);", txt)
    lib = ctypes.CDLL(pfmi.build())
    for s in NEW:
        assert s in SYMBOLS and hasattr(lib, s)


# ---- MixtureModel host logic against a stand-in engine -------------------------------------------------------------------------------
class FakeEngine:
    """the part of Engine that MixtureModel uses: component p's log density is -|x - m_p|^2 / 2 - p / 3; draws of (p, seed) are
    deterministic numbers; a refit bumps the token"""

    def __init__(self, d, name):
        self.d, self.name, self.gen, self.calls = d, name, 0, []

    def fit_token(self):
        return (0, self.gen)

    def check_token(self, token, what):
        import pfmi
        if token != self.fit_token():
            raise pfmi.StaleHandleError(what)

    def mean_of(self, p):
        return np.arange(self.d) * 0.1 + p + (0.5 if self.name == "b" else 0.0)

    def comp(self, p, X):
        return -0.5 * np.sum((X - self.mean_of(p)[:, None]) ** 2, axis=0) - p / 3

    def mixture_logpdf(self, points, X, componentwise=False):
        self.calls.append(list(points))
        C = np.stack([self.comp(p, X) for p in points], axis=1)
        lse = logsumexp(C, axis=1)
        return (lse, C) if componentwise else lse

    def draws(self, p, seed, n):
        X = np.add.outer(np.full(self.d, 1000.0 * p + (seed % 997)), np.arange(n, dtype=np.float64))
        return X, None, None


def _mixture(engs, layout):
    import pfmi
    comps = [pfmi.MvNormal(engs[g].mean_of(p), None, engs[g], p, -1, engs[g].fit_token()) for g, p in layout]
    return pfmi.MixtureModel(comps)


def test_mixture_model_is_the_component_list():
    import pfmi
    e = FakeEngine(3, "a")
    mix = _mixture([e], [(0, 1), (0, 4), (0, 2)])
    assert isinstance(mix, list) and mix.ncomponents == 3 and len(mix) == 3
    assert all(a is b for a, b in zip(mix.components, mix))
    np.testing.assert_array_equal(mix.probs, np.full(3, 1 / 3))
    np.testing.assert_array_equal(mix.mean(), np.mean(np.stack([e.mean_of(p) for p in (1, 4, 2)]), axis=0))
    assert [c.point for c in mix] == [1, 4, 2]
    assert isinstance(pfmi.MixtureModel([]), list)


def test_engine_blocks_logaddexp_and_normalisation():
    ea, eb = FakeEngine(4, "a"), FakeEngine(4, "b")
    layout = [(0, 3), (0, 5), (0, 3), (1, 1), (1, 7)]          # multipathfinder's contiguous blocks; a repeated point
    mix = _mixture([ea, eb], layout)
    X = np.asfortranarray(np.random.default_rng(2).normal(size=(4, 9)) + 3)
    lp = mix.logpdf(X)
    assert ea.calls == [[3, 5, 3]] and eb.calls == [[1, 7]]    # one call per engine, its own components in order
    comp = np.stack([[ea, eb][g].comp(p, X) for g, p in layout], axis=1)
    want = np.logaddexp(logsumexp(comp[:, :3], axis=1), logsumexp(comp[:, 3:], axis=1)) - np.log(5)
    np.testing.assert_array_equal(lp, want)
    np.testing.assert_allclose(lp, logsumexp(comp, axis=1) - np.log(5), rtol=1e-14)
    np.testing.assert_array_equal(mix.componentwise_logpdf(X), comp)
    np.testing.assert_array_equal(mix.pdf(X), np.exp(lp))
    assert mix.logpdf(X[:, 4]) == lp[4]
    np.testing.assert_array_equal(mix.componentwise_logpdf(X[:, 4]), comp[4])


def test_rand_ids_and_seeds():
    import pfmi
    ea, eb = FakeEngine(2, "a"), FakeEngine(2, "b")
    layout = [(0, 0), (0, 2), (1, 1)]
    mix = _mixture([ea, eb], layout)
    X, ids = mix.rand(pfmi.HostRNG(5), 40)
    rng = pfmi.HostRNG(5)
    u = rng.rand(40)
    np.testing.assert_array_equal(ids, np.minimum(np.floor(3 * u).astype(np.int64), 2) + 1)
    seeds = rng.rand_u64(3)                                    # always K seeds, after the n uniforms
    assert X.shape == (2, 40) and ids.dtype == np.int64 and set(ids) <= {1, 2, 3}
    for k, (g, p) in enumerate(layout):
        cols = np.flatnonzero(ids == k + 1)
        np.testing.assert_array_equal(X[:, cols], [ea, eb][g].draws(p, int(seeds[k]), len(cols))[0])


def test_stale_component_raises():
    import pfmi
    ea, eb = FakeEngine(2, "a"), FakeEngine(2, "b")
    mix = _mixture([ea, eb], [(0, 0), (1, 1)])
    X = np.zeros((2, 3))
    mix.logpdf(X)
    eb.gen += 1                                                # engine b was refitted
    for op in (lambda: mix.logpdf(X), lambda: mix.componentwise_logpdf(X), lambda: mix.mean(),
               lambda: mix.rand(pfmi.HostRNG(1), 4), lambda: mix.pdf(X)):
        with pytest.raises(pfmi.StaleHandleError):
            op()


# ---- the main mixture kernel stays in registers --------------------------------------------------------------------------------------
def _mfma_kernel_resources(kpad, stage):
    sys.path.insert(0, os.path.join(ROOT, "pathfinder.jl_amd", "tools"))
    import kernel_resources as kr
    import pfmi
    pfmi.build()
    t = kr.kernel_resources()
    hits = [k for k in t if k.startswith(f"pf_mixture_mfma_kernel<{kpad}, {stage}>(")]
    assert len(hits) == 1, hits
    r = t[hits[0]]
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    assert r["vgpr_count"] <= 256, r                           # two waves per SIMD (512-thread workgroups)
    return r


@pytest.mark.parametrize("kpad", [12, 20])
@pytest.mark.parametrize("stage", ["true", "false"])
def test_mixture_mfma_kernel_has_no_scratch(kpad, stage):
    _mfma_kernel_resources(kpad, stage)


# with the rows above: every instantiation the launcher can reach, (4,T) (8,T) (12,T) (16,T) (16,F) (20,T) (20,F) (32,T) (32,F)
# (kpad <= 12 always stages at d <= 1024: <4|8|12, false> are compiled but never launched)
@pytest.mark.parametrize("kpad,stage", [(4, "true"), (8, "true"), (16, "true"), (16, "false"), (32, "true"), (32, "false")])
def test_mixture_mfma_kernel_reachable_instantiations_have_no_scratch(kpad, stage):
    _mfma_kernel_resources(kpad, stage)
