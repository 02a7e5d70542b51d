"""Compare the device assembly of two trees kernel by kernel: the method behind profiles/prims_isa.txt and profiles/ransac_split_isa.txt.
usage: isa_compare.py [--rename OLD=NEW]... [--lines N] PARENT_DIR BRANCH_DIR      (each holds lr_X.s of every translation unit: hipcc <flags of
                                                  csrc/Makefile> --cuda-device-only -S lr_X.hip -o lr_X.s)
A translation unit present on both sides is compared as a whole file (__hip_cuid_<hash> masked).  Every kernel is then looked up by
its name wherever it lives: its text from the label to .Lfunc_end with the .amdhsa_kernel descriptor, the function's index within its
file masked in the labels (BB<n>_, .Lfunc_begin/end<n>, .Ltmp<n>), and its resource lines.
--rename OLD=NEW (repeatable): the parent's kernel whose demangled name begins with OLD is compared with the branch's one kernel whose
demangled name begins with NEW, each side's own symbol masked, instead of being listed as MISSING and NEW.
--lines N: print the differing lines of a kernel of equal length in which at most N lines differ (default 8)."""
import os, re, subprocess, sys

RES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy", "codeLenInByte")


def mask(line):
    line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", line)
    line = re.sub(r"\bL?BB\d+_", "BBn_", line)
    line = re.sub(r"[ \t]+;", " ;", line)      # (a label's comment is padded to a column: an index with more digits shortens the padding)
    return re.sub(r"\.L(func_begin|func_end|tmp)\d+", r".L\1n", line)


def kernels(path):
    """name -> (masked text, resources) of every kernel of an assembly file"""
    lines = open(path).read().split("\n")
    spills = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s+\.name:\s+(\S+)$", l)
        if m:
            spills[m.group(1)] = next(x.split(":")[1].strip() for x in lines[i:i + 8] if ".sgpr_spill_count" in x)
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"(_Z\w+):\s", lines[i])
        if not m or m.group(1) not in spills:
            i += 1
            continue
        name, j = m.group(1), i
        while not re.match(r"\.Lfunc_end\d+:", lines[j]): j += 1
        res = {}
        for l in lines[j:j + 40]:
            r = re.match(r"; (\w+)[:=]? *=? *(\d+)", l)
            if r and r.group(1) in RES: res.setdefault(r.group(1), r.group(2))
        res["sgpr_spill_count"] = spills[name]
        out[name] = ([mask(l) for l in lines[i:j + 1]], res)
        i = j + 1
    return out


def demangle(name):
    return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().replace("void ", "", 1)


args, renames, show = sys.argv[1:], [], 8
while args and args[0] in ("--rename", "--lines"):
    if args[0] == "--lines": show = int(args[1])
    else: renames.append(tuple(args[1].split("=", 1)))
    args = args[2:]
pa, br = args
fa, fb = sorted(f for f in os.listdir(pa) if f.endswith(".s")), sorted(f for f in os.listdir(br) if f.endswith(".s"))
print("# 1. whole files")
whole = set()      # the files that are identical as a whole
for f in fa:
    if f not in fb: print(f"{f[:-2]}.hip: parent only"); continue
    a, b = ([mask(l) for l in open(os.path.join(d, f)).read().split("\n")] for d in (pa, br))
    nd = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
    if nd == 0: whole.add(f)
    print(f"{f[:-2]}.hip: " + (f"identical ({len(a)} lines)" if nd == 0 else f"{nd} differing lines of {len(a)}: see 2."))
print("#\n# 2. kernel by kernel, wherever the kernel lives")
ka = {n: (f, k) for f in fa for n, k in kernels(os.path.join(pa, f)).items()}
kb = {n: (f, k) for f in fb for n, k in kernels(os.path.join(br, f)).items()}
renamed = {}      # parent symbol -> branch symbol
for old, new in renames:
    src, dst = [n for n in ka if demangle(n).startswith(old)], [n for n in kb if demangle(n).startswith(new)]
    if len(src) != 1 or len(dst) != 1: sys.exit(f"--rename {old}={new}: {len(src)} kernels in the parent, {len(dst)} on the branch, expected one each")
    renamed[src[0]] = dst[0]
bad = 0
for f in fa:
    names = [n for n, (g, _) in ka.items() if g == f]
    if f in whole and all(kb.get(n, ("",))[0] == f for n in names) and [n for n, (g, _) in kb.items() if g == f] == names: continue      # identical file, same kernels: covered by 1.
    print(f"{f[:-2]}: {len(names)} kernels in the parent")
    for n in names:
        (_, (ta, ra)) = ka[n]
        m = renamed.get(n, n)
        if m not in kb: print(f"  MISSING    {demangle(n)}"); bad += 1; continue
        g, (tb, rb) = kb[m]
        if m != n: ta, tb = [l.replace(n, "KERNEL") for l in ta], [l.replace(m, "KERNEL") for l in tb]
        same = ta == tb and ra == rb
        bad += not same
        nd = sum(x != y for x, y in zip(ta, tb)) + abs(len(ta) - len(tb))
        print(f"  {'identical' if same else 'differs  '}  {demangle(n)}  -> " + (f"{demangle(m)} in " if m != n else "") + f"{g[:-2]}.hip  ({len(ta)} lines" + ("" if same else f", {nd} differ") + ")")
        if not same and len(ta) == len(tb) and nd <= show:      # a handful of lines: show them
            for x, y in zip(ta, tb):
                if x != y: print(f"      parent: {x.strip()}\n      branch: {y.strip()}")
        for side, r in (("parent", ra), ("branch", rb)):
            if not same or side == "branch":
                print(f"      {side}: VGPRs {r.get('NumVgprs')} SGPRs {r.get('TotalNumSgprs')} LDS {r.get('LDSByteSize')} scratch {r.get('ScratchSize')} occupancy {r.get('Occupancy')}"
                      f" sgpr_spill_count {r['sgpr_spill_count']} code bytes {r.get('codeLenInByte')}" + (" (= parent)" if same else ""))
extra = [n for n in kb if n not in ka and n not in renamed.values()]
for n in extra: print(f"  NEW        {demangle(n)}  in {kb[n][0][:-2]}.hip")
print(f"# {len(ka)} kernels in the parent, {len(kb)} on the branch; {bad} differ or are missing, {len(extra)} new")
sys.exit(1 if bad or extra else 0)
