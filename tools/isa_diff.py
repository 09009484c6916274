#!/usr/bin/env python3
"""Per-kernel ISA tables of two source trees, side by side: registers, scratch, static LDS, spills and the count of instructions by mnemonic.

    tools/isa_diff.py TREE_A TREE_B [file.hip ...] [--keep DIR] [--show SUBSTRING ...]

Each tree's powerserve_amd/build.py gives the flags (FLAGS, NOSLP) and the variants a file is built in (default, -DPS_CONTRACT=1, -DPS_TIMELINE=1);
every (file, variant) is compiled with --cuda-device-only -S and the assembly is read.  Prints one summary line per (file, variant), one line for every kernel symbol
that differs (a kernel present on one side only is a difference) and, with --show, the figures of the kernels whose demangled name contains a substring; exits 1 on any
difference.  --keep DIR keeps the .s files (DIR/a, DIR/b) and reuses one when its compile command is the same and it is newer than every source of its tree."""
import collections, importlib.util, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

FILES = ["k_gemv4.hip", "k_gemvb.hip", "k_gemvk.hip", "k_gemv6.hip", "k_gemv.hip", "k_qkvattn.hip", "k_attn.hip", "k_attn_long.hip", "k_gemm4k.hip"]
KEYS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count"]


def tree_build(tree):
    spec = importlib.util.spec_from_file_location("ps_build_" + re.sub(r"\W", "_", tree), os.path.join(tree, "powerserve_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_tree(tree, out, files):
    b = tree_build(tree)
    os.makedirs(out, exist_ok=True)
    hdrs = [os.path.join(b.CSRC, f) for f in os.listdir(b.CSRC) if f.endswith(".h")]
    jobs, res = [], []
    for f in files:
        for tag, on, d in (("default", True, []), ("contract", f in b.CONTRACT_SOURCES, ["-DPS_CONTRACT=1"]), ("timeline", f in b.TIMELINE_SOURCES, ["-DPS_TIMELINE=1"])):
            if not on:
                continue
            src, s = os.path.join(b.CSRC, f), os.path.join(out, f"{f[:-4]}.{tag}.s")
            cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *b.FLAGS, *(["-fno-slp-vectorize"] if f in b.NOSLP else []), *d, "--cuda-device-only", "-S", src, "-o", s]
            res.append((f"{f} [{tag}]", s))
            try:
                fresh = open(s + ".cmd").read() == " ".join(cmd) and all(os.path.getmtime(x) <= os.path.getmtime(s) for x in [src] + hdrs)
            except OSError:
                fresh = False
            if not fresh:
                jobs.append(cmd)

    def run(cmd):
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        open(cmd[-1] + ".cmd", "w").write(" ".join(cmd))

    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(run, jobs))
    return res


def read_asm(path):
    """{kernel symbol: {key: value, "ops": Counter of mnemonics}}"""
    lines = open(path).read().splitlines()
    kernels = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m}
    tab, cur = {}, None
    for l in lines:
        m = re.match(r"(\w+):", l)
        if m and m.group(1) in kernels:
            cur = tab.setdefault(m.group(1), {"ops": collections.Counter()})["ops"]
        elif l.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and l.startswith("\t") and not l.lstrip().startswith((".", ";")):
            cur[l.split()[0]] += 1
    # the metadata note: one "  - " entry per kernel with its keys sorted by name (.agpr_count and .group_segment_fixed_size stand BEFORE .name)
    start = lines.index("amdhsa.kernels:")
    entry = None
    for l in lines[start + 1:] + ["  - .end: 0"]:
        if l.startswith("  - ") or not l.startswith(" "):
            if entry is not None:
                missing = [k for k in KEYS if k not in entry and not k.endswith("spill_count")]
                if entry.get(".name") not in tab or missing:
                    raise SystemExit(f"{path}: metadata entry {entry.get('.name')} has no code or lacks {missing}")
                tab[entry[".name"]].update({k: entry.get(k, "0") for k in KEYS})
            if not l.startswith("  - "):
                break
            entry, l = {}, "    " + l[4:]
        m = re.match(r"    (\.\w+):\s*(\S+)", l)
        if m and entry is not None:
            entry[m.group(1)] = m.group(2)
    lacking = [s for s in tab if ".vgpr_count" not in tab[s]]
    if lacking or set(tab) != kernels:
        raise SystemExit(f"{path}: kernels without metadata or code: {lacking or kernels ^ set(tab)}")
    return tab


def demangle(syms):
    out = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    return {s: d.replace("(anonymous namespace)::", "").split("(")[0] for s, d in zip(syms, out)}


def figures(k):
    return (f"vgpr {k['.vgpr_count']} agpr {k['.agpr_count']} sgpr {k['.sgpr_count']} scratch {k['.private_segment_fixed_size']} lds {k['.group_segment_fixed_size']} "
            f"spills {k['.vgpr_spill_count']}/{k['.sgpr_spill_count']} insts {sum(k['ops'].values())}")


def main():
    args, keep, show = sys.argv[1:], None, []
    while "--keep" in args:
        i = args.index("--keep"); keep = args[i + 1]; del args[i:i + 2]
    while "--show" in args:
        i = args.index("--show"); show.append(args[i + 1]); del args[i:i + 2]
    tree_a, tree_b, files = os.path.abspath(args[0]), os.path.abspath(args[1]), (args[2:] or FILES)
    tmp = keep or tempfile.mkdtemp(prefix="isa_diff_")
    ra, rb = compile_tree(tree_a, os.path.join(tmp, "a"), files), compile_tree(tree_b, os.path.join(tmp, "b"), files)
    n_diff = n_kernels = 0
    for (title, sa), (_, sb) in zip(ra, rb):
        ta, tb = read_asm(sa), read_asm(sb)
        names = demangle(sorted(set(ta) | set(tb)))
        rows, nd = [], 0
        for sym in sorted(names, key=names.get):
            ka, kb = ta.get(sym), tb.get(sym)
            if ka is None or kb is None:
                nd += 1
                rows.append(f"  {names[sym]}: only in {'B' if ka is None else 'A'}")
                continue
            d = [f"{key[1:]} {ka[key]} -> {kb[key]}" for key in KEYS if ka[key] != kb[key]]
            d += [f"{op} {ka['ops'][op]} -> {kb['ops'][op]}" for op in sorted(set(ka["ops"]) | set(kb["ops"])) if ka["ops"][op] != kb["ops"][op]]
            nd += bool(d)
            if d:
                rows.append(f"  {names[sym]}: {figures(ka)} | DIFFERS: " + ", ".join(d))
            elif any(s in names[sym] for s in show):
                rows.append(f"  {names[sym]}: {figures(ka)} | same")
        n_kernels += len(names); n_diff += nd
        print(f"== {title}: {len(ta)} / {len(tb)} kernels, {sum(sum(k['ops'].values()) for k in ta.values())} / {sum(sum(k['ops'].values()) for k in tb.values())} instructions, {nd} differ")
        print("\n".join(rows) if rows else "", end="\n" if rows else "")
    print(f"{n_kernels} kernel symbols, {n_diff} differ")
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
