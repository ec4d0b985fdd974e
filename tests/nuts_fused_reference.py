"""What the tests of the fused NUTS kernel (pathfinder.jl_amd/csrc/nuts_fused_kernel.hip) share.  Not collected by pytest; used by
tests/test_gpu_nuts_fused_steps.py / test_gpu_nuts_fused.py and pinned on the CPU by tests/test_nuts_fused_reference_cpu.py.

No new bound is defined here.  The transition is nuts_reference's (mirror, check: the bounds of its docstring); the in-kernel target
evaluation is hmc_fused_reference's (target_ratios: the bound of its docstring); both are asserted at ratio <= 1.  This file holds the
case grids, the plan names and the test hook of the launch cap."""
import hmc_fused_reference as F
import hmc_reference as H
import nuts_reference as N

ROUNDS_CAP = F.ROUNDS_CAP            # HM_FUSED_ROUNDS (pathfinder.jl_amd/csrc/hmc_rows.h): the cap is shared with fused static HMC
KINDS = {"dir+", "dir-", "subtree_turn", "tree_turn", "max_depth", "divergent", "candidate_replaced", "candidate_kept"}

# ---- the grid of tests/test_gpu_nuts_fused_steps.py: hmc_fused_reference.GRID (22 cases), max_depth 5, T = 3, K = 3 -------------------
GRID = F.GRID
GRID_DEPTH, GRID_T, GRID_K = 5, 3, 3
case_id = F.case_id


def plan_name(tg, d, kpad):
    """the plan counter nuts_fused:<KPAD>:<res|stream>:<f|g0|g8|g16> of one launch"""
    return "nuts_fused:%d:%s:%s" % (kpad, "res" if H.resident(d, kpad) else "stream", F.target_tag(tg))


def grid_plans(pfmi):
    return {plan_name(F.grid_target(pfmi, tn, d), d, H.kpad_for(J)) for d, J, tn in GRID}


# the two shapes of the bit-identity tests (K = 4, max_depth 5, T = 20; adaptive: W = 12, T = 8)
BIT_CASES = F.BIT_CASES
BIT_K, BIT_DEPTH, BIT_T, BIT_W, BIT_TA = 4, 5, 20, 12, 8
BIT_CAPS = (None, 1, 7)              # the default cap, the rounds schedule, and a cap that cuts trees


def set_round_cap(pfmi, cap):
    """the test hook PFMI_NUTS_FUSED_ROUNDS (include/pfmi.h: pfmi_debug_set); None: the library's own cap"""
    L = pfmi._lib.lib()
    assert L.pfmi_debug_set(b"PFMI_NUTS_FUSED_ROUNDS", None if cap is None else str(int(cap)).encode()) == 0


def launches_bound(trips, cap):
    """[fewest, most] launches of a call whose slowest chain made `trips` trips: the pump issues at most its window (4) ahead of the last
    progress word it has read"""
    n = -(-trips // cap)
    return n, n + 4


assert N.GRID_DEPTH == GRID_DEPTH and N.GRID_T == GRID_T and N.GRID_K == GRID_K
