"""Per-block instruction issue of the ELBO scan's steady-state block loop, read from the compiler's gfx950 assembly.

    python tools/qf_issue_count.py [--asm FILE.s] [KC TGT RPAD NG ...]  -> table per instantiation (default: 12 1 8 2, the config-3 scan)

The scan (`csrc/elbo_qf_kernel.hip`) is issue bound: on gfx950 the f64 MFMA co-issues with nothing, so a block's time is the sum of
its MFMA, VALU, LDS and scalar issue (profiles/r02_coissue_microbench.txt).  The MFMA part of a block is fixed by the contraction
(4 k-steps x NG groups x (NT [+ NT] [+ TR]) 4x4x4 MFMAs); everything else on the steady-state path is overhead this tool counts.

How the steady-state path is found: `hipcc -S` of the kernel source (the library's flags), the kernel's text cut at its symbol, basic
blocks at `.LBB` labels and `; %bb.` markers, loop membership from LLVM's `; in Loop: Header=` / `This Inner Loop Header` comments.
A steady trip of a loop is its cheapest path from the header back to the header that still issues the most 4x4x4 MFMAs and no
16x16x4 MFMA: the rare sides of the block loop -- the inverse-CDF fix-up (probability 2^-19 per normal), the priority switch every
QF_PRIO_FAIR blocks, the first / second / last block -- all add issue, so the cheapest full-work path is the interior block whatever
the code layout.  The steady loop is the loop whose trip carries the most 4x4x4 MFMAs, and among those the cheapest; a trip may cover
several blocks (unrolling), the counts are divided down to one 16-row block.

The cycle estimate weighs each class by its issue cost for one wave's stream on one SIMD (approximate, from the project's
co-issue micro-benchmark and the MI355X constants: 32-bit VALU / f64 VALU / LDS / VMEM 4, 64-bit integer multiply 8, scalar 1,
`s_nop N` N + 1 wait states); it is a guide for comparing builds, not a prediction of the kernel's time.
"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
SRC = os.path.join(PKG, "csrc", "elbo_qf_kernel.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S"]

HEADLINE = (12, 1, 8, 2)
CLASSES = ("mfma4", "mfma16", "valu_f64", "mad_u64", "mov_b64", "valu32", "lds", "vmem", "smem", "salu", "nop_cycles", "waitcnt",
           "branch")
WEIGHT = {"valu_f64": 4, "mad_u64": 8, "mov_b64": 4, "valu32": 4, "lds": 4, "vmem": 4, "smem": 1, "salu": 1, "waitcnt": 1, "branch": 1,
          "nop_cycles": 1}


def compile_asm(src=SRC, extra=()):
    """device assembly of the scan's translation unit (all instantiations) as text"""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "qf.s")
        subprocess.run([HIPCC, *FLAGS, *extra, "-I", os.path.dirname(src), src, "-o", out], check=True, capture_output=True, text=True)
        return open(out).read()


def mangled(kc, tgt, rpad, ng):
    return f"_Z17pf_elbo_qf_kernelILi{kc}ELi{tgt}ELi{rpad}ELi{ng}EEv8ElboArgsiiiiiiiPdPjji"


def kernel_lines(asm, sym):
    lines = asm.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def classify(ins):
    op = ins.split()[0]
    if op.startswith("v_mfma"):
        return "mfma16" if "16x16" in op else "mfma4"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op == "s_nop":
        return "nop_cycles"
    if op == "s_waitcnt" or op.startswith("s_waitcnt_"):
        return "waitcnt"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_mad_u64_u32") or op.startswith("v_mad_i64_i32"):
        return "mad_u64"
    if op.startswith("v_mov_b64"):
        return "mov_b64"
    if op.startswith("v_") and "_f64" in op and not op.startswith("v_cvt_"):
        return "valu_f64"
    if op.startswith("v_"):
        return "valu32"
    return None


def parse_blocks(klines):
    """[(name, header_or_None, [instructions])] in layout order; `header` is the innermost loop header's name"""
    fn = None
    for l in klines:
        m = re.match(r"^\.LBB(\d+)_\d+:", l)
        if m:
            fn = m.group(1)
            break
    blocks = []
    cur = None
    for l in klines:
        m = re.match(r"^\.L(BB\d+_\d+):(.*)$", l) or re.match(r"^; %bb\.(\d+):(.*)$", l)
        if m:
            name = m.group(1) if m.group(1).startswith("BB") else f"BB{fn}_{m.group(1)}"
            rest = m.group(2)
            cur = [name, None, []]
            h = re.search(r"Header=(BB\d+_\d+)", rest)
            if h:
                cur[1] = h.group(1)
            blocks.append(cur)
            continue
        if cur is None:
            continue
        if "This Inner Loop Header" in l or "This Loop Header" in l:
            cur[1] = cur[0]
            continue
        s = l.strip()
        if not s or s.startswith((";", ".")):
            continue
        cur[2].append(s.split(";")[0].strip())
    return blocks


def steady_trip(blocks, header):
    """instructions of one steady trip of the loop headed by `header` (see the module docstring)"""
    pos = {b[0]: i for i, b in enumerate(blocks)}
    members = {b[0] for b in blocks if b[1] == header}
    memo = {}

    def key(ins):
        c = count(ins)
        return (c["mfma4"] - 1000 * c["mfma16"], -non_mfma_cycles(c))

    def best(i):
        # best (key, instructions) from the top of block i back to the header; the loop body minus its back edges is acyclic
        if i in memo:
            return memo[i]
        memo[i] = None                                   # (guards against a cycle that bypasses the header)
        name, _, ins = blocks[i]
        cands = []
        for j, s in enumerate(ins):
            op = s.split()[0]
            if op.startswith("s_cbranch") or op == "s_branch":
                tgt = re.sub(r"^\.L", "", s.split()[-1])
                head = ins[:j + 1]
                if tgt == header:
                    cands.append(head)
                elif tgt in members:
                    r = best(pos[tgt])
                    if r is not None:
                        cands.append(head + r[1])
                if op == "s_branch":
                    break
            if op == "s_endpgm":
                break
        else:
            if i + 1 < len(blocks) and blocks[i + 1][0] in members:
                r = best(i + 1) if blocks[i + 1][0] != header else (None, [])
                if r is not None:
                    cands.append(ins + r[1])
        out = max(((key(c), c) for c in cands), key=lambda t: t[0], default=None)
        memo[i] = out
        return out

    r = best(pos[header])
    if r is None:
        raise RuntimeError(f"no trip of {header} returns to the header")
    return r[1]


def count(ins):
    c = dict.fromkeys(CLASSES, 0)
    for s in ins:
        k = classify(s)
        if k == "nop_cycles":
            c[k] += int(s.split()[1], 0) + 1
        elif k:
            c[k] += 1
    return c


def mfma4_per_block(kc, tgt, rpad, ng):
    nt, tr = kc // 4, rpad // 4
    per_row = nt + (nt if tgt != 0 else 0) + (tr if tgt == 1 else 0)
    return 4 * ng * per_row


def non_mfma_cycles(c):
    return sum(WEIGHT[k] * c[k] for k in WEIGHT)


def steady_counts(asm, kc=12, tgt=1, rpad=8, ng=2):
    """per-block class counts of the steady-state block loop of pf_elbo_qf_kernel<kc, tgt, rpad, ng>"""
    blocks = parse_blocks(kernel_lines(asm, mangled(kc, tgt, rpad, ng)))
    headers = sorted({b[1] for b in blocks if b[1] is not None and b[1] == b[0]})
    want = mfma4_per_block(kc, tgt, rpad, ng)
    best = None
    for h in headers:
        try:
            trip = steady_trip(blocks, h)
        except (RuntimeError, KeyError):
            continue
        c = count(trip)
        if c["mfma4"] == 0 or c["mfma4"] % want:
            continue
        key = (c["mfma4"] // want > 0, c["mfma4"] / max(1, c["mfma4"] // want), -non_mfma_cycles(c) / (c["mfma4"] // want))
        if best is None or key > best[0]:
            best = (key, h, c)
    if best is None:
        raise RuntimeError(f"no steady block loop found in pf_elbo_qf_kernel<{kc}, {tgt}, {rpad}, {ng}>")
    _, h, c = best
    nb = c["mfma4"] // want
    per = {k: v / nb for k, v in c.items()}
    per["blocks_per_trip"] = nb
    per["header"] = h
    per["non_mfma_cycles"] = non_mfma_cycles(c) / nb
    per["mfma_cycles"] = 16 * per["mfma4"] + 64 * per["mfma16"]
    return per


def prologue_load_trips(asm, kc=12, tgt=1, rpad=8, ng=2):
    """(dependent global round trips, global loads) of the kernel's prologue: its text in layout order from the entry to the first
    `s_barrier`.  A trip is an `s_waitcnt` with a vmcnt field whose next vector-memory event is a further `global_load`: the kernel
    waited for what was in flight and then sent more.  One flight of loads, however many waits drain it, counts 0; a loop counts once."""
    trips = loads = 0
    waited = False
    for l in kernel_lines(asm, mangled(kc, tgt, rpad, ng))[1:]:
        s = l.strip().split(";")[0].strip()
        if not s or s.startswith("."):
            continue
        op = s.split()[0]
        if op == "s_barrier":
            return trips, loads
        if op == "s_waitcnt" and "vmcnt" in s:
            waited = True
        elif op.startswith("global_load"):
            loads += 1
            trips += waited
            waited = False
    raise RuntimeError("no s_barrier in the kernel")


FINISH_CLASSES = ("mfma16", "mfma4", "lds_reads", "scratch_loads", "nop_cycles", "waitcnt", "cross_lane", "waits_in_chain",
                  "reads_in_chain")


def finish_counts(asm, kc=12, tgt=1, rpad=8, ng=2):
    """counts of the per-batch draw finish of pf_elbo_qf_kernel<kc, tgt, rpad, ng>, tgt != 0: the kernel's text in layout order from its
    last `s_barrier` (the end of the publish step) to `s_endpgm`, which is the finish of all `ng` groups of a wave and the batch loop's
    latch.  `per_group` divides by ng.  waits_in_chain / reads_in_chain: `s_waitcnt`s / LDS reads that sit between the first and the last
    MFMA of a stretch of the region that ends in a group's stores -- inside the dependency chains, where their latency is on the path"""
    ins = []
    for l in kernel_lines(asm, mangled(kc, tgt, rpad, ng))[1:]:
        s = l.strip().split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        if s.split()[0] == "s_barrier":
            ins = []
            continue
        ins.append(s)
        if s.split()[0] == "s_endpgm":
            break
    c = dict.fromkeys(FINISH_CLASSES, 0)
    # a group's stores end its chains: the span from the first to the last MFMA is taken per stretch between global stores
    seg, segs = 0, []
    for s in ins:
        segs.append(seg)
        seg += s.startswith("global_store")
    span = {}
    for i, s in enumerate(ins):
        if s.startswith("v_mfma"):
            span[segs[i]] = (span.get(segs[i], (i, i))[0], i)
    for i, s in enumerate(ins):
        op = s.split()[0]
        k = classify(s)
        lo, hi = span.get(segs[i], (0, -1))
        if k in ("mfma16", "mfma4", "waitcnt"):
            c[k] += 1
        elif k == "nop_cycles":
            c[k] += int(s.split()[1], 0) + 1
        if op.startswith("ds_read"):
            c["lds_reads"] += 1
            c["reads_in_chain"] += lo < i < hi
        if op.startswith("scratch_load") or (op.startswith("buffer_load") and "offen" in s):
            c["scratch_loads"] += 1
        if op.startswith(("v_permlane", "ds_swizzle", "ds_bpermute", "ds_permute")) or "row_" in s or "quad_perm" in s:
            c["cross_lane"] += 1
        if k == "waitcnt" and lo < i < hi:
            c["waits_in_chain"] += 1
    c["per_group"] = {k: v / ng for k, v in c.items()}
    return c


def main(argv):
    asm_file = None
    if argv[:1] == ["--asm"]:
        asm_file, argv = argv[1], argv[2:]
    nums = [int(a) for a in argv]
    insts = [tuple(nums[i:i + 4]) for i in range(0, len(nums), 4)] or [HEADLINE]
    asm = open(asm_file).read() if asm_file else compile_asm()
    for inst in insts:
        r = steady_counts(asm, *inst)
        print(f"pf_elbo_qf_kernel<{', '.join(map(str, inst))}>: steady loop {r['header']}, {r['blocks_per_trip']} block(s) per trip; per block:")
        for k in CLASSES:
            print(f"  {k:12s} {r[k]:7.1f}")
        print(f"  {'~cycles':12s} MFMA {r['mfma_cycles']:.0f} + other {r['non_mfma_cycles']:.0f}")
        t, n = prologue_load_trips(asm, *inst)
        print(f"  prologue: {n} global loads, {t} dependent round trip(s) behind the first flight")
        if inst[1] != 0:
            f = finish_counts(asm, *inst)
            print("  finish, per group: " + ", ".join(f"{k} {f['per_group'][k]:g}" for k in FINISH_CLASSES))


if __name__ == "__main__":
    main(sys.argv[1:])
