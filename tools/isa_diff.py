#!/usr/bin/env python3
"""Compare the gfx950 code generation of two source trees, kernel by kernel (host only: compiles, runs nothing).

  tools/isa_diff.py OLD_TREE NEW_TREE csrc/mfgpu_kernels_g.hip csrc/mfgpu_pass2.hip ... [--old-only FILE ...]

Every listed .hip file (path relative to the package directory dealii-cuda_amd/ of a tree) is compiled to device
assembly in both trees with the flags of the Makefile plus -S --offload-device-only
-Rpass-analysis=kernel-resource-usage.  Files given with --old-only exist in OLD_TREE only (their kernels moved into
one of the listed files).  Kernels are matched by their demangled name and template arguments; where the name changed,
by the template arguments alone (an old kernel also matches the new one that has its arguments plus a trailing 1: a
width parameter added with the old behaviour at 1).  Per kernel one line:

  identical                 same resources and, comments / directives / local label numbers aside, same instructions
  resources equal           ... but the instruction streams differ: both instruction counts are printed
  DIFFERENT                 the resources that differ, old -> new, and both instruction counts

Resources: VGPRs, AGPRs, SGPRs, scratch bytes per lane, occupancy (waves per SIMD) and static LDS bytes, as the
assembler's per-kernel summary states them.  Exit status 1 if any kernel is DIFFERENT or unmatched.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--offload-device-only", "-S",
         "-Rpass-analysis=kernel-resource-usage"]
RESOURCES = [("VGPRs", "NumVgprs"), ("AGPRs", "NumAgprs"), ("SGPRs", "TotalNumSgprs"), ("scratch", "ScratchSize"),
             ("occupancy", "Occupancy"), ("LDS", "LDSByteSize")]


def compile_asm(tree, rel, out, extra):
    src = os.path.join(tree, "dealii-cuda_amd", rel)
    cmd = [os.environ.get("HIPCC", "hipcc")] + FLAGS + extra + [src, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.exit("%s\n%s" % (" ".join(cmd), r.stderr[-4000:]))
    return out


def demangle(names):
    if not names:
        return {}
    tool = next((t for t in ("llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt", "c++filt")
                 if subprocess.run(["sh", "-c", "command -v " + t], stdout=subprocess.DEVNULL).returncode == 0), None)
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names) + "\n", stdout=subprocess.PIPE, text=True).stdout.split("\n")
    return dict(zip(names, out))


def split_name(dem):
    """'void ns::f<a, b<c>>(args)' -> ('f', ('a', 'b<c>'))"""
    s = re.sub(r"^void ", "", dem)
    depth, end = 0, len(s)
    for i, ch in enumerate(s):  # cut the parameter list: the first '(' outside <> that is not '(anonymous namespace)'
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0 and not s.startswith("(anonymous namespace)", i):
            end = i
            break
    s = s[:end]
    lt = s.find("<")
    if lt < 0:
        return s.split("::")[-1], ()
    name, args, depth, cur = s[:lt].split("::")[-1], [], 0, ""
    for ch in s[lt + 1:s.rfind(">")]:
        if ch == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
            continue
        depth += ch == "<"
        depth -= ch == ">"
        cur += ch
    args.append(cur.strip())
    return name, tuple(args)


def kernels_of(asm_path):
    """{mangled name: (resources dict, [normalised instructions])} of the kernels (.amdhsa_kernel) of an assembly file"""
    text = open(asm_path).read()
    kernel_names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out = {}
    for name in kernel_names:
        m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
        if not m:
            continue
        ins = []
        for line in m.group(1).split("\n"):
            line = line.split(";")[0].strip()
            if re.match(r"\.LBB\d+_\d+:", line):
                ins.append(".LBB:")
                continue
            if not line or line.startswith("."):
                continue
            line = re.sub(r"\.LBB\d+_\d+", ".LBB", line)
            line = re.sub(r"\s+", " ", line)
            ins.append(line)
        tail = text[m.end():m.end() + 4000]
        res = {}
        for label, key in RESOURCES:
            r = re.search(r";\s*%s:\s*(\d+)" % key, tail)
            res[label] = int(r.group(1)) if r else -1
        out[name] = (res, ins)
    return out


def count(ins):
    return sum(1 for i in ins if not i.endswith(":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--old-only", nargs="*", default=[], help="files of OLD_TREE whose kernels moved into the listed files")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--keep", help="directory for the assembly files (default: a temporary one)")
    ap.add_argument("--reuse-old", action="store_true", help="with --keep: do not recompile OLD_TREE files already there")
    ap.add_argument("-D", action="append", default=[], help="extra macro for both compiles")
    a = ap.parse_args()
    tmp = None if a.keep else tempfile.TemporaryDirectory()
    keep = a.keep or tmp.name
    os.makedirs(keep, exist_ok=True)
    extra = ["-D" + d for d in a.D]
    jobs = []
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        for side, tree, files in (("old", a.old_tree, a.files + a.old_only), ("new", a.new_tree, a.files)):
            for f in files:
                out = os.path.join(keep, side + "_" + os.path.basename(f) + ".s")
                if side == "old" and a.reuse_old and os.path.exists(out):
                    continue
                jobs.append(ex.submit(compile_asm, tree, f, out, extra))
        for j in jobs:
            j.result()
    old, new = {}, {}
    for side, files, into in (("old", a.files + a.old_only, old), ("new", a.files, new)):
        for f in files:
            ks = kernels_of(os.path.join(keep, side + "_" + os.path.basename(f) + ".s"))
            dem = demangle(sorted(ks))
            for k, v in ks.items():
                into[split_name(dem[k])] = v
    pairs, unmatched_new = [], dict(new)
    rest = []
    for key in sorted(old):
        if key in unmatched_new:
            pairs.append((key, key))
            del unmatched_new[key]
        else:
            rest.append(key)
    bad = 0
    for key in rest:  # renamed, or a trailing width parameter of 1 added
        cand = [k for k in unmatched_new
                if k[1] == key[1] + ("1",) and k[0] == key[0]] or [k for k in unmatched_new if k[1] == key[1] and key[1]]
        if len(cand) == 1:
            pairs.append((key, cand[0]))
            del unmatched_new[cand[0]]
        else:
            print("%s<%s>: no counterpart in the new tree" % (key[0], ", ".join(key[1])))
            bad += 1
    for key in sorted(unmatched_new):
        print("%s<%s>: only in the new tree" % (key[0], ", ".join(key[1])))
        bad += 1
    n_ident = 0
    for ko, kn in sorted(pairs):
        (ro, io), (rn, i_n) = old[ko], new[kn]
        title = "%s<%s>" % (kn[0], ", ".join(kn[1]))
        if ko != kn:
            title += " (was %s<%s>)" % (ko[0], ", ".join(ko[1]))
        diff = ["%s %d -> %d" % (l, ro[l], rn[l]) for l, _ in RESOURCES if ro[l] != rn[l]]
        if diff:
            print("%s: DIFFERENT %s; instructions %d -> %d" % (title, ", ".join(diff), count(io), count(i_n)))
            bad += 1
        elif io != i_n:
            print("%s: resources equal (%s), instructions %d -> %d" %
                  (title, " ".join("%s %d" % (l, rn[l]) for l, _ in RESOURCES), count(io), count(i_n)))
        else:
            print("%s: identical" % title)
            n_ident += 1
    print("%d kernels compared, %d identical" % (len(pairs), n_ident))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
