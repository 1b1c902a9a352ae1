"""What the compiler made of the channel-leg kernels of the mixed batches (needs hipcc, no GPU) -> profiles/r10_mix_chan_isa.txt.

  1. with --parent-csrc DIR (the csrc directory of the parent commit, include/ beside it as in the tree): the device assembly of the
     three units the per-symbol code was moved out of (nrldpc_modem, nrldpc_awgn, nrldpc_channel), old against new, lines containing
     __hip_cuid dropped -- moving text into headers must not change an existing kernel;
  2. registers, scratch and occupancy of every kernel of the two new units and of the single kernels beside them, from the compiler's
     -Rpass-analysis=kernel-resource-usage remarks;
  3. the floating-point instructions of the fused mix kernel against those of the five single fused kernels it switches between,
     opcode by opcode: both are compiled with contraction allowed, and the mix kernel equals the single ones bit for bit only if the
     same multiply-adds were fused (v_fma / v_fmac / v_pk_fma against v_mul + v_add).

    python tools/isa_mix_chan.py [--parent-csrc DIR] [--out profiles/r10_mix_chan_isa.txt]
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import importlib  # noqa: E402

build = importlib.import_module("ldpc-3gpp-matlab_amd.build")
OLD_UNITS = ("nrldpc_modem", "nrldpc_awgn", "nrldpc_channel")
NEW_UNITS = ("nrldpc_mix_modem", "nrldpc_mix_chan")
FP = re.compile(r"^v_(pk_)?(fma|fmac|mad|mac|mul|add|sub|subrev|max|min|exp|log|sqrt|rsq|rcp|sin|cos|fract|ldexp|cvt|div\w*)_\w*f(32|16)")


def compile_unit(csrc, unit, out_dir):
    """(assembly text, remarks text) of the device pass of one unit, with the library's flags"""
    s = os.path.join(out_dir, unit + ".s")
    cmd = [build._hipcc(), *build.FLAGS, "-I" + os.path.join(os.path.dirname(os.path.dirname(csrc)), "include"), "-I" + csrc,
           "--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, unit + ".hip"), "-o", s]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(r.stderr)
    return open(s).read(), r.stderr


def kernels(asm):
    """{mangled name: [instruction mnemonics]}"""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and re.match(r"^\t[vs]_|^\t(global|buffer|flat|ds)_", line):
            cur.append(line.split()[0])
    return out


def fp_hist(ins):
    return collections.Counter(re.sub(r"_(e32|e64|dpp|sdwa)$", "", i) for i in ins if FP.match(i))


def resources(remarks):
    """[(kernel, {field: value})] from the resource-usage remarks"""
    out = []
    for line in remarks.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            out.append((m.group(1), {}))
            continue
        m = re.search(r"remark: .*?\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and out:
            out[-1][1][m.group(1)] = int(m.group(2))
    return out


def demangled(name):
    r = subprocess.run(["c++filt", name], capture_output=True, text=True)
    return (r.stdout.strip() or name).replace("nrldpc::", "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-csrc", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_mix_chan_isa.txt"))
    args = ap.parse_args()
    lines = ["Channel leg of the mixed batches (nrldpc_mix_modem.hip, nrldpc_mix_chan.hip, nrldpc_mix_chan.h): what the compiler made of it",
             "=" * 120, "", "tool: tools/isa_mix_chan.py; flags: " + " ".join(build.FLAGS) + " (device pass only)", ""]
    with tempfile.TemporaryDirectory() as tmp:
        new = {u: compile_unit(build.CSRC, u, tmp) for u in OLD_UNITS + NEW_UNITS}
        lines += ["1. The three units the per-symbol code was moved out of, against the parent commit", ""]
        if args.parent_csrc:
            os.makedirs(os.path.join(tmp, "parent"))
            drop = lambda t: [x for x in t.splitlines() if "__hip_cuid" not in x]  # noqa: E731
            for u in OLD_UNITS:
                old = compile_unit(os.path.abspath(args.parent_csrc), u, os.path.join(tmp, "parent"))
                lines.append("%-16s %3d kernels, whole file identical (cuid lines dropped): %s" % (u + ".s", len(kernels(new[u][0])), drop(old[0]) == drop(new[u][0])))
        else:
            lines.append("(not compared: no --parent-csrc given)")
        lines += ["", "2. Registers, scratch, occupancy (compiler's resource-usage remarks; wave64, 512 VGPRs per SIMD lane)", "",
                  "%-92s %5s %5s %8s %10s %5s" % ("kernel", "SGPR", "VGPR", "scratch", "waves/SIMD", "LDS")]
        for u in NEW_UNITS + OLD_UNITS:
            lines.append("-- %s.hip" % u)
            for name, r in resources(new[u][1]):
                lines.append("%-92s %5d %5d %8d %10d %5d" % (demangled(name)[:92], r.get("TotalSGPRs", -1), r.get("VGPRs", -1), r.get("ScratchSize [bytes/lane]", -1),
                                                             r.get("Occupancy [waves/SIMD]", -1), r.get("LDS Size [bytes/block]", -1)))
        scratch = [r.get("ScratchSize [bytes/lane]", -1) for u in NEW_UNITS for _, r in resources(new[u][1])]
        lines += ["", "scratch of every kernel of the two new units is 0: %s" % all(x == 0 for x in scratch), "",
                  "3. Floating-point instructions: the fused mix kernel against the five single fused kernels (contraction allowed in both)", ""]
        single = {k: fp_hist(v) for k, v in kernels(new["nrldpc_channel"][0]).items() if "awgn_llr_kernel" in k}
        (mk, mv), = [(k, v) for k, v in kernels(new["nrldpc_mix_chan"][0]).items() if "awgn_llr_kernel" in k]
        mix, total = fp_hist(mv), collections.Counter()
        for h in single.values():
            total += h
        ops = sorted(set(mix) | set(total))
        lines.append("%-16s" % "opcode" + "".join("%8s" % ("Q_m %s" % re.search(r"ILi(\d)E", k).group(1)) for k in single) + "%10s%10s" % ("sum", "mix"))
        for op in ops:
            lines.append("%-16s" % op + "".join("%8d" % h.get(op, 0) for h in single.values()) + "%10d%10d" % (total.get(op, 0), mix.get(op, 0)))
        lines += ["", "the mix kernel's floating-point instructions are, opcode by opcode, the sum of the five single kernels': %s" % (mix == total),
                  "(the same multiply-adds are fused: v_fma_f32, v_fmac_f32, v_pk_fma_f32 counts agree; the integer and address code differs, as it must)"]
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0 if mix == total and all(x == 0 for x in scratch) else 1


if __name__ == "__main__":
    sys.exit(main())
