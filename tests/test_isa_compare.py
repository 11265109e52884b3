"""tools/isa_compare.py: its text handling on two short assembly snippets (no compiler): comments and label numbers do not count, a
changed immediate counts as differing lines under an identical opcode sequence, a rename is followed, and the conditions it exits on."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location("isa_compare", os.path.join(os.path.dirname(__file__), "..", "tools", "isa_compare.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)


def _kernel(name, fn, first_label, imm, comment, vgpr_spill=0, vgprs=6):
    asm = f"""
\t.protected\t{name} ; -- Begin function {name}
\t.globl\t{name}
\t.type\t{name},@function
{name}:           ; @{name}
; %bb.0:
\ts_load_dwordx2 s[0:1], s[0:1], {imm}   ; {comment}
\ts_waitcnt lgkmcnt(0)
\ts_cbranch_execz .LBB{fn}_{first_label + 1}
.LBB{fn}_{first_label}:                 ; =>This Inner Loop Header: Depth=1
\tv_add_u32_e32 v0, 1, v0
\ts_cbranch_scc1 .LBB{fn}_{first_label}
.LBB{fn}_{first_label + 1}:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr {vgprs}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{fn}:
"""
    r = "x.hip:1:1: remark:     "
    remarks = f"x.hip:1:1: remark: Function Name: {name} [-Rpass-analysis=kernel-resource-usage]\n" + "".join(
        f"{r}{key}: {val} [-Rpass-analysis=kernel-resource-usage]\n" for key, val in (
            ("TotalSGPRs", 10), ("VGPRs", vgprs), ("AGPRs", 0), ("ScratchSize [bytes/lane]", 0), ("Dynamic Stack", "False"),
            ("Occupancy [waves/SIMD]", 8), ("SGPRs Spill", 0), ("VGPRs Spill", vgpr_spill), ("LDS Size [bytes/block]", 0)))
    return asm, remarks


def _build(*kernels, demangled={}):
    asm, remarks = ("".join(part) for part in zip(*kernels))
    return isa.kernels_of(asm, remarks, names=lambda mangled: {n: demangled.get(n, n) for n in mangled})


def _row(rows, name):
    return next(r for r in rows if r.startswith(name + " |"))


def test_comments_and_label_numbers_do_not_count():
    old = _build(_kernel("k_a", 0, 1, "0x1c8", "kernarg"), _kernel("k_b", 1, 4, "0x10", "x"))
    new = _build(_kernel("k_b", 0, 2, "0x10", "another comment"), _kernel("k_a", 1, 7, "0x1c8", "moved behind k_b"))
    assert old["k_a"][1][0] == "s_load_dwordx2 s[0:1], s[0:1], 0x1c8" and len(old["k_a"][1]) == 8
    assert old["k_a"][0] == {"TotalSGPRs": 10, "VGPRs": 6, "AGPRs": 0, "ScratchSize [bytes/lane]": 0, "Occupancy [waves/SIMD]": 8,
                             "SGPRs Spill": 0, "VGPRs Spill": 0, "LDS Size [bytes/block]": 0}
    rows, ok = isa.compare(old, new, must_match=["k_a", "k_b"])
    assert ok and _row(rows, "k_a").endswith("| 8 | identical") and _row(rows, "k_b").endswith("| identical")
    assert "only in parent: none; only in new: none" in rows[0]


def test_a_changed_immediate_is_differing_lines_with_the_same_opcodes():
    old, new = _build(_kernel("k_a", 0, 1, "0x1c8", "")), _build(_kernel("k_a", 0, 1, "0x1d0", ""))
    rows, ok = isa.compare(old, new)
    assert ok and _row(rows, "k_a").endswith("2 differing lines (parent: 8 lines); opcode sequence: identical")
    rows, ok = isa.compare(old, new, must_match=["k_a"])
    assert not ok and "MUST MATCH" in _row(rows, "k_a")
    # another instruction is another opcode sequence
    other = {"k_a": (new["k_a"][0], [l.replace("v_add_u32_e32", "v_sub_u32_e32") for l in new["k_a"][1]])}
    assert "opcode sequence: differs" in _row(isa.compare(old, other)[0], "k_a")


def test_a_rename_is_followed():
    old = _build(_kernel("k_noise_cap", 0, 1, "0x10", ""), _kernel("k_gone", 1, 1, "0x10", ""))
    new = _build(_kernel("_Z7k_noiseILb1ELb0EEvv", 0, 3, "0x10", ""), _kernel("k_new", 1, 1, "0x10", ""),
                 demangled={"_Z7k_noiseILb1ELb0EEvv": "k_noise<true, false>"})
    rows, ok = isa.compare(old, new, {"k_noise_cap": "k_noise<true, false>"}, ["k_noise<true, false>"])
    assert ok and _row(rows, "k_noise<true, false>").endswith("| identical") and _row(rows, "k_new").endswith("| new")
    assert "only in parent: k_gone; only in new: k_new" in rows[0]
    rows, ok = isa.compare(old, new, must_match=["k_noise<true, false>"])   # without the map the kernel has no parent
    assert not ok


def test_template_arguments_survive_an_anonymous_namespace():
    # the argument list is the bracket that closes at the end, whatever stands in front of the name or inside the list
    assert isa.short_name("void (anonymous namespace)::k_tower_sb<4, true>(unsigned char const*, int)") == "k_tower_sb<4, true>"
    assert isa.short_name("void (anonymous namespace)::k_tower_sb<4, false>(unsigned char const*, int)") == "k_tower_sb<4, false>"
    assert isa.short_name("void k_noise<true, false>()") == "k_noise<true, false>"
    assert isa.short_name("k_foo(int (*)(), int)") == "k_foo" and isa.short_name("_Zunknown") == "_Zunknown"
    # two mangled names that differ only in a template argument are two kernels, with or without a demangler on the machine
    a, b = "_ZN12_GLOBAL__N_110k_tower_sbILi4ELb1EEEvPKhi", "_ZN12_GLOBAL__N_110k_tower_sbILi4ELb0EEEvPKhi"
    names = isa.demangle([a, b])
    assert names[a] != names[b]
    assert (names[a], names[b]) in ((a, b), ("k_tower_sb<4, true>", "k_tower_sb<4, false>"))
    both = isa.kernels_of("".join(_kernel(n, i, 1, "0x10", "")[0] for i, n in enumerate((a, b))), "")
    assert sorted(both) == sorted(names.values())


def _with_mfma(kernel, head, tail):
    """the snippet's loop body gets an MFMA; `head` / `tail` = immediates in front of it (line 1) and behind it"""
    res, text = kernel
    at = text.index("v_add_u32_e32 v0, 1, v0")
    return res, ["s_load_dwordx2 s[0:1], s[0:1], %s" % head] + text[1:at] + ["v_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]",
                                                                              "v_add_u32_e32 v0, %s, v0" % tail] + text[at + 1:]


def test_from_the_first_mfma_on():
    base = _build(_kernel("k_a", 0, 1, "0x10", ""))["k_a"]
    old = {"k_a": _with_mfma(base, "0x10", 1), "k_b": _with_mfma(base, "0x10", 1)}
    new = {"k_a": _with_mfma(base, "0x18", 1), "k_b": _with_mfma(base, "0x10", 2)}   # k_a differs in front of the MFMA, k_b behind it
    assert isa.first_mfma(old["k_a"][1]) == 5 and isa.first_mfma(base[1]) == 0
    assert isa.line_diff(old["k_a"][1], new["k_a"][1]) == (2, 1, 1) and isa.line_diff(old["k_b"][1], new["k_b"][1]) == (2, 6, 6)
    rows, ok = isa.compare(old, new, from_mfma=["k_a"])
    assert ok and "parent's last differing line 1, its first v_mfma 5: 2 differing lines" in _row(rows, "k_a")
    assert "parent's last differing line 6, its first v_mfma 5" in _row(rows, "k_b")
    rows, ok = isa.compare(old, new, from_mfma=["k_a", "k_b"])
    assert not ok and "MUST MATCH FROM THE FIRST MFMA" in _row(rows, "k_b") and "MUST MATCH" not in _row(rows, "k_a")
    # a line that only the new text has, behind ITS first MFMA, counts as well; so does the MFMA line itself
    longer = {"k_a": (base[0], new["k_a"][1] + ["s_nop 0"])}
    assert not isa.compare(old, longer, from_mfma=["k_a"])[1]
    moved = {"k_a": (base[0], [l.replace("a[0:3], v[0:3]", "a[0:3], v[8:11]") for l in old["k_a"][1]])}
    assert not isa.compare(old, moved, from_mfma=["k_a"])[1]
    # identical text passes; a kernel without an MFMA has to match as a whole; a missing kernel fails
    assert isa.compare(old, old, from_mfma=["k_a", "k_b"])[1]
    plain_old, plain_new = _build(_kernel("k_a", 0, 1, "0x10", "")), _build(_kernel("k_a", 0, 1, "0x18", ""))
    assert not isa.compare(plain_old, plain_new, from_mfma=["k_a"])[1] and isa.compare(plain_old, plain_old, from_mfma=["k_a"])[1]
    assert not isa.compare(old, new, from_mfma=["k_c"])[1]


def test_a_resource_number_or_a_vgpr_spill_fails():
    old = _build(_kernel("k_a", 0, 1, "0x10", ""))
    rows, ok = isa.compare(old, _build(_kernel("k_a", 0, 1, "0x10", "", vgprs=7)))
    assert not ok and "RESOURCES DIFFER (parent: VGPR 6)" in _row(rows, "k_a")
    spilled = _build(_kernel("k_a", 0, 1, "0x10", "", vgpr_spill=3))
    rows, ok = isa.compare(spilled, spilled)
    assert not ok and "VGPR SPILL" in _row(rows, "k_a")


def test_the_makefile_flags_are_read_not_restated():
    flags = isa.cxxflags(os.path.join(os.path.dirname(__file__), "..", "alphazero-risk_amd", "csrc", "Makefile"))
    assert "--offload-arch=gfx950" in flags and "-ffp-contract=off" in flags and "-O3" in flags
