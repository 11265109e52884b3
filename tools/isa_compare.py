#!/usr/bin/env python3
"""Device code of two source trees (or two git revisions) side by side, without a GPU: the check behind "no change to the kernels".

    tools/isa_compare.py OLD NEW [--file azr_engine.hip ...] [--rename 'k_old = k_new<true, false>' ...] [--must-match KERNEL ...]
                         [--must-match-from-mfma KERNEL ...]

OLD and NEW are directories holding a checkout, or git revisions, which are exported to temporary directories.  The named .hip files
of alphazero-risk_amd/csrc are cross-compiled for gfx950 with that tree's own Makefile CXXFLAGS plus `--cuda-device-only -S
-Rpass-analysis=kernel-resource-usage`, once as the product build and once with -DAZR_TEST_HOOKS.  Per kernel the resource remarks are
compared, and the instruction text with comments dropped and block labels renumbered in order of appearance; "differing lines" counts
the lines of a line diff, "opcode sequence" compares the mnemonics alone.  For a kernel that differs, the last differing line of the
parent's text and the parent's first v_mfma line are printed too: code in front of a kernel's first MFMA runs once per launch.  Kernels
are named as the demangler prints them, without the argument list and without `(anonymous namespace)::`.  A compile, not a run.

Exit status 1 if a --must-match kernel differs in instruction text (or is missing), a --must-match-from-mfma kernel differs at or
behind the first v_mfma line of either text (or anywhere, if it has no MFMA; or is missing), a kernel of both trees differs in a
resource number, or any kernel spills a VGPR.
"""
import argparse, difflib, os, re, shlex, subprocess, sys, tarfile, tempfile

CSRC = os.path.join("alphazero-risk_amd", "csrc")
RES = [("VGPRs", "VGPR"), ("AGPRs", "AGPR"), ("TotalSGPRs", "SGPR"), ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "LDS"),
       ("Occupancy [waves/SIMD]", "occupancy"), ("SGPRs Spill", "SGPR spills"), ("VGPRs Spill", "VGPR spills")]


def kernel_text(asm):
    """{mangled kernel name: its lines, from the entry label to the end of the function}"""
    lines, out = asm.splitlines(), {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M):
        start = next(i for i, l in enumerate(lines) if l.split(";")[0].strip() == name + ":")
        end = next(i for i in range(start, len(lines)) if re.match(r"\s*\.section\b|\.Lfunc_end", lines[i]))
        out[name] = lines[start + 1:end]
    return out


def normalise(lines):
    """comments and blank lines dropped, local labels (.LBB3_7 and the like) renumbered in order of appearance"""
    seen = {}
    body = [l.split(";")[0].strip() for l in lines]
    return [re.sub(r"\.L\w+", lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), l) for l in body if l]


def opcodes(lines):
    return [l.split()[0] for l in lines if not l.endswith(":")]


def line_diff(a, b):
    """(differing lines of the line diff, 1-based number of the last differing line of `a`, of `b`) — 0 where a text has none"""
    ops = [o for o in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes() if o[0] != "equal"]
    return (sum((i2 - i1) + (j2 - j1) for _, i1, i2, j1, j2 in ops), max([i2 for _, i1, i2, _, _ in ops if i2 > i1], default=0),
            max([j2 for _, _, _, j1, j2 in ops if j2 > j1], default=0))


def first_mfma(lines):
    """1-based number of the first line starting with v_mfma, 0 if there is none"""
    return next((i + 1 for i, l in enumerate(lines) if l.startswith("v_mfma")), 0)


def resources(remarks):
    """{mangled kernel name: {remark key: number}} from the compiler's kernel-resource-usage remarks"""
    out, cur = {}, None
    for l in remarks.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", l)
        if not m: continue
        if m.group(1) == "Function Name": cur = out.setdefault(m.group(2), {})
        elif cur is not None and m.group(2).isdigit(): cur[m.group(1)] = int(m.group(2))
    return out


def short_name(demangled):
    """`void (anonymous namespace)::k_name<4, true>(unsigned char const*, int)` -> `k_name<4, true>`: the argument list is the
    bracket that closes at the end of the name, not everything from the first bracket on"""
    d = demangled.strip()
    if d.endswith(")"):
        depth = 0
        for i in range(len(d) - 1, -1, -1):
            depth += (d[i] == ")") - (d[i] == "(")
            if depth == 0:
                d = d[:i]
                break
    return re.sub(r"^void ", "", d).replace("(anonymous namespace)::", "")


def demangle(names):
    """mangled -> `k_name<args>` if a demangler is on the machine, else the mangled name"""
    for tool in ("c++filt", "llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt"):
        try:
            res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        except (OSError, subprocess.CalledProcessError):
            continue
        return {n: short_name(d) for n, d in zip(names, res)}
    return {n: n for n in names}


def kernels_of(asm, remarks, names=demangle):
    """{kernel name: (resource numbers, normalised instruction lines)} of one compiled file"""
    text, res = kernel_text(asm), resources(remarks)
    nm = names(list(text))
    return {nm[k]: (res.get(k, {}), normalise(v)) for k, v in text.items()}


def compare(old, new, renames=None, must_match=(), from_mfma=()):
    """(report lines, ok) for two kernels_of() dictionaries; `renames` maps a name of `old` to its name in `new`"""
    old = {(renames or {}).get(k, k): v for k, v in old.items()}
    ok, rows = True, []
    for k in sorted(new):
        res, text = new[k]
        row = "%s | %s | %s, %s | %d | " % (k, " ".join(str(res.get(r, "?")) for r, _ in RES[:6]), res.get("SGPRs Spill", "?"), res.get("VGPRs Spill", "?"), len(text))
        if res.get("VGPRs Spill", 0): ok, row = False, row + "VGPR SPILL; "
        if k not in old:
            rows.append(row + "new")
            continue
        ores, otext = old[k]
        if ores != res:
            ok, row = False, row + "RESOURCES DIFFER (parent: %s); " % ", ".join("%s %s" % (s, ores.get(r, "?")) for r, s in RES if ores.get(r) != res.get(r))
        if otext == text: row += "identical"
        else:
            n, olast, last = line_diff(otext, text)
            omfma, mfma = first_mfma(otext), first_mfma(text)
            row += "parent's last differing line %d, its first v_mfma %s: %d differing lines (parent: %d lines); opcode sequence: %s" % (
                olast, omfma or "none", n, len(otext), "identical" if opcodes(otext) == opcodes(text) else "differs")
            if k in must_match: ok, row = False, row + "; MUST MATCH"
            if k in from_mfma and (not omfma or not mfma or olast >= omfma or last >= mfma): ok, row = False, row + "; MUST MATCH FROM THE FIRST MFMA"
        rows.append(row)
    gone = sorted(set(old) - set(new))
    for k in list(must_match) + list(from_mfma):
        if k not in new or k not in old: ok = False; rows.append("%s | must match, but is not in both trees" % k)
    head = "%d kernels in the parent, %d in the new build; only in parent: %s; only in new: %s" % (
        len(old), len(new), ", ".join(gone) or "none", ", ".join(sorted(set(new) - set(old))) or "none")
    return [head, "# kernel | " + " ".join(s for _, s in RES[:6]) + " | SGPR spills, VGPR spills | instruction lines | identical or differing lines"] + rows, ok


def cxxflags(makefile):
    """the Makefile's CXXFLAGS, with its own $(ARCH)"""
    text = open(makefile).read().replace("\\\n", " ")
    var = lambda v: re.search(r"^%s\s*[:?]?=\s*(.*)$" % v, text, re.M).group(1)
    return shlex.split(var("CXXFLAGS").replace("$(ARCH)", var("ARCH")))


def compile_tree(root, files, hooks, hipcc):
    out = {}
    csrc = os.path.join(root, CSRC)
    for f in files:
        with tempfile.TemporaryDirectory() as tmp:
            s = os.path.join(tmp, "out.s")
            cmd = [hipcc] + cxxflags(os.path.join(csrc, "Makefile")) + (["-DAZR_TEST_HOOKS"] if hooks else []) + [
                "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", f, "-o", s]
            p = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
            if p.returncode: sys.exit("%s failed in %s:\n%s" % (" ".join(cmd), csrc, p.stderr))
            out.update(kernels_of(open(s).read(), p.stderr))
    return out


def tree_of(spec, stack):
    """a directory as it is; a git revision exported (plain `git archive`) to a temporary directory"""
    if os.path.isdir(spec): return spec
    tmp = tempfile.TemporaryDirectory()
    stack.append(tmp)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    git = subprocess.Popen(["git", "-C", repo, "archive", spec, "alphazero-risk_amd/csrc", "include"], stdout=subprocess.PIPE)
    with tarfile.open(fileobj=git.stdout, mode="r|") as tar: tar.extractall(tmp.name)
    if git.wait(): sys.exit("git archive %s failed" % spec)
    return tmp.name


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old"); ap.add_argument("new")
    ap.add_argument("--file", action="append", help="a .hip file of alphazero-risk_amd/csrc (default: azr_engine.hip)")
    ap.add_argument("--rename", action="append", default=[], metavar="'OLD = NEW'", help="a parent kernel's name in the new tree")
    ap.add_argument("--must-match", action="append", default=[], metavar="KERNEL", help="new-tree name of a kernel that has to be instruction-identical")
    ap.add_argument("--must-match-from-mfma", action="append", default=[], metavar="KERNEL",
                    help="new-tree name of a kernel that may differ only in front of its first v_mfma line")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    renames = dict(tuple(s.strip() for s in r.split("=", 1)) for r in a.rename)
    keep, ok = [], True
    old, new = tree_of(a.old, keep), tree_of(a.new, keep)
    for hooks, title in ((False, "product build (libazr_hip.so)"), (True, "hook build (libazr_hip_test.so, -DAZR_TEST_HOOKS)")):
        rows, good = compare(compile_tree(old, a.file or ["azr_engine.hip"], hooks, a.hipcc),
                             compile_tree(new, a.file or ["azr_engine.hip"], hooks, a.hipcc), renames, a.must_match, a.must_match_from_mfma)
        ok = ok and good
        print("# %s: %s" % (title, rows[0]))
        print("\n".join(rows[1:]))
        print("# conditions (must-match kernels identical, from-mfma kernels identical from their first MFMA on, the parent's kernels keep their resource numbers, no VGPR spill): %s\n" % ("hold" if good else "VIOLATED"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
