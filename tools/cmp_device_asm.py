"""Compare the gfx950 device code of kernel sources between a git revision and the working tree, kernel by kernel (no GPU needed).

    python tools/cmp_device_asm.py [--base REV] [--rename 'REGEX=>REPL' ...] fused_ws.hip wide.hip ...
    python tools/cmp_device_asm.py gemm.hip                                  # one source against HEAD: "35 kernels", every line `identical`

Each source under dgnn_amd/csrc is compiled twice with the Makefile's flags plus --cuda-device-only -S: once from REV (default HEAD,
unpacked with git archive) and once from the working tree.  Kernels are paired by demangled name; --rename rewrites base names first
(for template parameters that were removed).  For each pair it reports whether the instruction stream is identical after branch labels
are renumbered, and the register, LDS and scratch figures of both sides.  Kernels present on one side only are listed."""
import argparse
import io
import os
import re
import shutil
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dgnn_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
          "private_segment_fixed_size")


def makefile_flags(src_dir, name):
    text = open(os.path.join(src_dir, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    m = re.search(r"^FLAGS_%s\s*=\s*(.*)$" % re.escape(name), text, re.M)
    return flags + (m.group(1).split() if m else [])


def compile_s(src_dir, name, out):
    cmd = [HIPCC] + makefile_flags(src_dir, name) + ["--cuda-device-only", "-S", os.path.join(src_dir, name + ".hip"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    return open(out).read()


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt or not names:
        return {n: n for n in names}
    res = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, res))


def kernels(asm):
    """mangled name -> (normalised instruction list, {field: value})"""
    meta = {}
    md = asm[asm.index(".amdgpu_metadata"):]
    for entry in re.split(r"\n  - ", md)[1:]:
        m = re.search(r"^    \.name:\s+(\S+)", entry, re.M)
        if not m:  # amdhsa.version and the like
            continue
        name = m.group(1)
        meta[name] = {f: int(m.group(1)) if (m := re.search(r"^    \.%s:\s+(\d+)" % f, entry, re.M)) else None for f in FIELDS}
    out = {}
    lines = asm.split("\n")
    for name in meta:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        labels, body = {}, []
        for l in lines[start + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            t = l.split(";", 1)[0].strip()
            if not t or t.startswith(".amdhsa") or t.startswith(".end_amdhsa") or t.startswith(".section") or t.startswith(".p2align"):
                continue
            for lab in re.findall(r"\.LBB\d+_\d+", t):
                labels.setdefault(lab, ".L%d" % len(labels))
            body.append(re.sub(r"\.LBB\d+_\d+", lambda m: labels[m.group(0)], t))
        out[name] = (body, meta[name])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default="HEAD")
    ap.add_argument("--rename", action="append", default=[], help="REGEX=>REPL applied to the base side's demangled names")
    ap.add_argument("sources", nargs="+", help="file names under dgnn_amd/csrc (with or without .hip)")
    a = ap.parse_args()
    rules = [tuple(r.split("=>", 1)) for r in a.rename]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        arch = subprocess.run(["git", "-C", ROOT, "archive", a.base, "dgnn_amd/csrc", "include"], check=True, capture_output=True).stdout
        tarfile.open(fileobj=io.BytesIO(arch)).extractall(tmp)
        base_dir = os.path.join(tmp, "dgnn_amd", "csrc")
        for src in a.sources:
            name = os.path.basename(src)[:-4] if src.endswith(".hip") else os.path.basename(src)
            kb = kernels(compile_s(base_dir, name, os.path.join(tmp, name + ".base.s")))
            kn = kernels(compile_s(CSRC, name, os.path.join(tmp, name + ".new.s")))
            db, dn = demangle(list(kb)), demangle(list(kn))
            new_by_name = {dn[m]: m for m in kn}
            seen = set()
            print("== %s: %d kernels at %s, %d in the working tree" % (name, len(kb), a.base, len(kn)))
            for mb in sorted(kb, key=lambda m: db[m]):
                nm = db[mb]
                for pat, rep in rules:
                    nm = re.sub(pat, rep, nm)
                if nm not in new_by_name:
                    print("  gone      %s" % db[mb])
                    continue
                mn = new_by_name[nm]
                seen.add(mn)
                (ib, fb), (inn, fn) = kb[mb], kn[mn]
                same = ib == inn and fb == fn
                bad += not same
                tag = "identical" if same else ("same-regs" if fb == fn else "DIFFERS")
                figs = " ".join("%s %s->%s" % (f.replace("_fixed_size", "").replace("_count", ""), fb[f], fn[f]) for f in FIELDS if fb[f] != fn[f])
                instr = "" if ib == inn else " (instructions %d -> %d, stream differs)" % (len(ib), len(inn))
                print("  %-9s %s%s%s%s" % (tag, db[mb], "" if nm == db[mb] else "  ->  " + nm, instr, ("  " + figs) if figs else ""))
            for mn in sorted(set(kn) - seen, key=lambda m: dn[m]):
                print("  new       %s" % dn[mn])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
