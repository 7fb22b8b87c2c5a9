"""Build-machine tool (no GPU): instruction census of the flagship ONF kernel, onf_x32_kernel<14,0,512,1>, per 32-sample
tile.  Compiles csrc/onf_x32_k14.hip to gfx950 assembly with the Makefile's flags (or reads --asm FILE), weights every
instruction by how often a tile executes it, and prints MFMA / VALU / DS / VMEM / SALU totals plus the classes of vector
instructions that form no result (profiles/k1_vector_diet.txt).

Weights.  The persistent chunk loop is the outermost loop that holds MFMAs: one trip = one tile per wave, weight 1; code
outside it (image copy, exit) counts 0.  Inside, the loops that hold MFMAs are, in program order, the rolled L1 block-pair
loop (FS / 2 - 2 = 4 trips at NKB 14) and the rolled L1^T tile loop (NMT - 1 = 6 trips).  The region skipped by the first
wave-uniform forward branch behind the chunk loop's header is the pose sampling, which runs every other chunk (weight 1/2).
Other forward branches are short and counted in full.

Usage: python tools/x32/isa_census.py [--asm FILE] [--kernel 14,0,512,1] [--keep-asm FILE]"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "pytorch-motion-planner_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-I" + os.path.join(ROOT, "include"),
         "-Wall", "-Wno-unused-function"]      # csrc/Makefile: FLAGS


def compile_asm(nkb, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc] + FLAGS + ["-S", "--cuda-device-only", os.path.join(CSRC, "onf_x32_k%d.hip" % nkb), "-o", out],
                   check=True, stderr=subprocess.DEVNULL)


def kernel_body(text, nkb, mode, xt, nt):
    name = "_ZN5nfopp3x3214onf_x32_kernelILi%dELi%dELi%dELi%dEEE" % (nkb, mode, xt, nt)
    lines, body, on = text.splitlines(), [], False
    for ln in lines:
        if not on and ln.startswith(name) and ":" in ln:
            on = True
            continue
        if on:
            if ln.startswith(".Lfunc_end"):
                break
            body.append(ln)
    if not body:
        sys.exit("kernel %s not found" % name)
    meta = {}
    at = text.find(".name:           " + name)
    for key in ("vgpr_count", "vgpr_spill_count", "sgpr_count"):      # (the metadata keys of a kernel are sorted: these follow .name)
        m = re.search(r"\." + key + r":\s+(\d+)", text[at:at + 900]) if at >= 0 else None
        meta[key] = int(m.group(1)) if m else None
    m = re.findall(r"\.agpr_count:\s+(\d+)", text[:at]) if at >= 0 else None             # ... and .agpr_count leads the entry
    meta["agpr_count"] = int(m[-1]) if m else None
    return body, meta


def parse(body):
    """-> [(mnemonic, operand string)] and {label: index of the instruction behind it}"""
    ins, labels = [], {}
    for ln in body:
        s = ln.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        if s.startswith("."):
            continue
        parts = s.split(None, 1)
        ins.append((parts[0], parts[1] if len(parts) > 1 else ""))
    return ins, labels


def weights(ins, labels, trips):
    is_mfma = [m.startswith("v_mfma") for m, _ in ins]
    loops = {}     # header index -> last index of a backward branch to it
    for i, (m, ops) in enumerate(ins):
        if m.startswith("s_cbranch") or m == "s_branch":
            t = labels.get(ops.strip())
            if t is not None and t <= i:
                loops[t] = max(loops.get(t, 0), i)
    with_mfma = sorted((a, b) for a, b in loops.items() if any(is_mfma[a:b + 1]))
    if not with_mfma:
        sys.exit("no loop holds MFMAs")
    chunk = max(with_mfma, key=lambda r: r[1] - r[0])
    inner = [r for r in with_mfma if r != chunk and chunk[0] <= r[0] and r[1] <= chunk[1]]
    if len(inner) != len(trips):
        sys.exit("expected %d rolled MFMA loops inside the chunk loop, found %d" % (len(trips), len(inner)))
    w = [0.0] * len(ins)
    for i in range(chunk[0], chunk[1] + 1):
        w[i] = 1.0
    for (a, b), n in zip(inner, trips):
        for i in range(a, b + 1):
            w[i] = float(n)
    first_mfma = next(i for i in range(chunk[0], chunk[1] + 1) if is_mfma[i])
    sampling = None
    for i in range(chunk[0], first_mfma):
        m, ops = ins[i]
        if m in ("s_cbranch_vccnz", "s_cbranch_vccz", "s_cbranch_scc0", "s_cbranch_scc1"):
            t = labels.get(ops.strip())
            if t is not None and i < t <= first_mfma and t - i > 100:
                sampling = (i + 1, t - 1)
                break
    if sampling:
        for i in range(sampling[0], sampling[1] + 1):
            w[i] *= 0.5
    return w, dict(chunk=chunk, inner=inner, sampling=sampling)


def literal(tok):
    tok = tok.strip()
    try:
        return int(tok, 0)
    except ValueError:
        return None


def census(ins, w, info):
    tot, cls = collections.Counter(), collections.Counter()
    l1t = info["inner"][-1]
    for i, (m, ops) in enumerate(ins):
        if w[i] == 0.0:
            continue
        if m.startswith("v_mfma"):
            tot["MFMA"] += w[i]
        elif m.startswith("v_"):
            tot["VALU"] += w[i]
        elif m.startswith("ds_"):
            tot["DS"] += w[i]
        elif m.split("_")[0] in ("buffer", "global", "flat", "scratch"):
            tot["VMEM"] += w[i]
        elif m.startswith("s_"):
            tot["SALU and control"] += w[i]
        if info["sampling"] and info["sampling"][0] <= i <= info["sampling"][1] and (m.startswith("v_") or m.startswith("s_")
                                                                                    or m.startswith("global") or m.startswith("buffer")):
            cls["sampling branch, all instructions (at weight 1/2)"] += w[i]
        if m == "s_nop":
            cls["s_nop"] += w[i]
        if m == "s_waitcnt":
            cls["s_waitcnt"] += w[i]
        if m in ("v_mov_b64_e32", "v_mov_b64", "v_pk_mov_b32"):
            cls["v_mov_b64 register-pair copies"] += w[i]
        if m in ("v_mov_b32_e32", "v_mov_b32") and re.match(r"^v\d+, v\d+$", ops):
            cls["v_mov_b32 v, v register copies"] += w[i]
        if m in ("v_add_u32_e32", "v_add_u32"):
            o = [t.strip() for t in ops.split(",")]
            lit = literal(o[1]) if len(o) == 3 else None
            if lit == 0:
                cls["v_add_u32 v, 0, v (copies)"] += w[i]
            elif lit is not None and lit > 0xffff:
                cls["v_add_u32 v, literal > 0xffff, v (LDS image offsets past a DS immediate)"] += w[i]
            elif lit is not None:
                cls["v_add_u32 v, other literal, v"] += w[i]
            elif len(o) == 3 and o[1].startswith("s") and l1t[0] <= i <= l1t[1]:
                cls["v_add_u32 v, s, v in the L1^T tile loop"] += w[i]
            elif len(o) == 3 and o[1].startswith("s"):
                cls["v_add_u32 v, s, v elsewhere"] += w[i]
            else:
                cls["v_add_u32 v, v, v"] += w[i]
    return tot, cls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", help="assembly of csrc/onf_x32_k<NKB>.hip (default: compile it)")
    ap.add_argument("--keep-asm", help="write the compiled assembly here")
    ap.add_argument("--kernel", default="14,0,512,1", help="NKB,MODE,XT,NT")
    a = ap.parse_args()
    nkb, mode, xt, nt = (int(v) for v in a.kernel.split(","))
    if a.asm:
        text = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            out = a.keep_asm or os.path.join(d, "k.s")
            compile_asm(nkb, out)
            text = open(out).read()
    fs = 12 if nkb >= 13 else 6
    trips = [fs // 2 - 2, (nkb + 1) // 2 - 1]
    body, meta = kernel_body(text, nkb, mode, xt, nt)
    ins, labels = parse(body)
    w, info = weights(ins, labels, trips)
    tot, cls = census(ins, w, info)
    print("onf_x32_kernel<%d,%d,%d,%d>: %d instructions in the kernel; registers %s" % (nkb, mode, xt, nt, len(ins), meta))
    print("loops: chunk %s, rolled MFMA loops %s x %s, sampling region %s" % (info["chunk"], info["inner"], trips, info["sampling"]))
    print("per 32-sample tile (weighted):")
    for k in ("MFMA", "VALU", "DS", "VMEM", "SALU and control"):
        print("  %-18s %8.1f" % (k, tot[k]))
    print("classes:")
    for k in sorted(cls):
        print("  %-78s %7.1f" % (k, cls[k]))


if __name__ == "__main__":
    main()
