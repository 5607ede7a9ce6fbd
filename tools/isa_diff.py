"""Compares the device code of two copies of rstnet_amd/csrc kernel by kernel (no GPU needed):

    python tools/isa_diff.py OLD_CSRC NEW_CSRC [--ablation] [--expect-removed PREFIX ...] [--expect-changed PREFIX ...]

Every .hip of both directories is compiled device-only to assembly with the flags of that directory's Makefile (--ablation: the tools
build, -DRST_ABLATION) and each function is reduced to its instruction stream: comments and directives stripped, local labels
renumbered in order of appearance.  Per file it reports the kernels whose demangled name exists on both sides (equal / differs), the
ones found on one side only that pair up with an equal stream (renamed), and what is left (added / removed).  The exit status is 0
only if every kernel is equal or renamed, except those whose name (as printed: without return type and anonymous namespace) starts
with an expected prefix: --expect-removed covers kernels that are gone, --expect-changed kernels whose stream differs, under the same
name or as one removed and one added.  The instruction text is compared, never searched."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LABEL = re.compile(r"\.L[\w$.]+")


def flags_of(csrc):
    """CXXFLAGS of the directory's Makefile, $(ARCH) filled in"""
    with open(os.path.join(csrc, "Makefile")) as f:
        mk = f.read()
    arch = re.search(r"^ARCH \?= *(\S+)", mk, re.M).group(1)
    return re.search(r"^CXXFLAGS := *(.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()


def compile_asm(job):
    csrc, name, out, extra = job
    r = subprocess.run([HIPCC, *flags_of(csrc), *extra, "--cuda-device-only", "-S", name, "-o", out], cwd=csrc, capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{os.path.join(csrc, name)}: compilation failed\n{r.stderr}")


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return {n: re.sub(r"^void ", "", d).replace("(anonymous namespace)::", "") for n, d in zip(names, out)}


def streams_of(path):
    """{demangled function name: instruction stream} of one assembly file"""
    with open(path) as f:
        lines = f.read().splitlines()
    funcs = {m.group(1) for ln in lines if (m := re.match(r"\s*\.type\s+(\S+),@function", ln))}
    out, cur, labels = {}, None, None
    for ln in lines:
        t = ln.split(";")[0].strip()
        if cur is None:
            if t.endswith(":") and t[:-1] in funcs:
                cur, labels = t[:-1], {}
                out[cur] = []
            continue
        if re.match(r"\.Lfunc_end\d+:", t):
            cur = None
            continue
        if not t or (t.startswith(".") and not t.endswith(":")):        # blank / comment only / directive
            continue
        out[cur].append(LABEL.sub(lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), t))
    names = demangle(sorted(out))
    return {names[k]: "\n".join(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--ablation", action="store_true", help="compare the tools build (-DRST_ABLATION)")
    ap.add_argument("--expect-removed", action="append", default=[], metavar="PREFIX")
    ap.add_argument("--expect-changed", action="append", default=[], metavar="PREFIX")
    ap.add_argument("--keep", metavar="DIR", help="leave the assembly files in DIR/old, DIR/new")
    a = ap.parse_args()
    extra = ["-DRST_ABLATION"] if a.ablation else []
    work = a.keep or tempfile.mkdtemp(prefix="isa_diff_")
    sides = {"old": os.path.abspath(a.old), "new": os.path.abspath(a.new)}
    files = {s: sorted(f for f in os.listdir(d) if f.endswith(".hip")) for s, d in sides.items()}
    jobs = []
    for s, d in sides.items():
        os.makedirs(os.path.join(work, s), exist_ok=True)
        jobs += [(d, f, os.path.join(work, s, f[:-4] + ".s"), extra) for f in files[s]]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        list(pool.map(compile_asm, jobs))

    def expected(name, prefixes):
        return any(name.startswith(p) for p in prefixes)

    total = {"equal": 0, "renamed": 0, "differ": 0, "added": 0, "removed": 0}
    bad = 0
    for f in sorted(set(files["old"]) | set(files["new"])):
        old = streams_of(os.path.join(work, "old", f[:-4] + ".s")) if f in files["old"] else {}
        new = streams_of(os.path.join(work, "new", f[:-4] + ".s")) if f in files["new"] else {}
        both = sorted(set(old) & set(new))
        differ = [k for k in both if old[k] != new[k]]
        removed, added, renamed = sorted(set(old) - set(new)), sorted(set(new) - set(old)), []
        for k in list(removed):
            twin = next((n for n in added if new[n] == old[k]), None)
            if twin:
                renamed.append((k, twin))
                removed.remove(k)
                added.remove(twin)
        n = {"equal": len(both) - len(differ), "renamed": len(renamed), "differ": len(differ), "added": len(added), "removed": len(removed)}
        print(f"{f}: " + ", ".join(f"{v} {k}" for k, v in n.items()))
        for k, twin in renamed:
            print(f"  renamed, equal stream: {k}\n                      -> {twin}")
        for k in differ:
            ok = expected(k, a.expect_changed)
            bad += not ok
            print(f"  differs{' (expected)' if ok else ''}: {k}")
        for k in removed:
            ok = expected(k, a.expect_removed + a.expect_changed)
            bad += not ok
            print(f"  removed{' (expected)' if ok else ''}: {k}")
        for k in added:      # (a kernel that changed its name AND its stream shows as one removed, one added)
            ok = expected(k, a.expect_changed)
            bad += not ok
            print(f"  added{' (expected)' if ok else ''}: {k}")
        for k, v in n.items():
            total[k] += v
    print(f"total, {len(set(files['old']) | set(files['new']))} files: " + ", ".join(f"{v} {k}" for k, v in total.items()) + f"; {bad} not expected")
    if not a.keep:
        shutil.rmtree(work)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
