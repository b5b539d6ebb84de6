"""CPU: the parsing and comparing half of tools/kernel_diff.py on two short canned listings (no compiler, no binutils).

Side A and side B hold four kernels: one identical, one whose only difference is a kernarg offset of an s_load, one with
another instruction, and one that is the same code under another symbol.  Plus one kernel that only B has.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import kernel_diff as KD  # noqa: E402

DIS_A = """
a.co:\tfile format elf64-amdgpu

Disassembly of section .text:

<_ZN12_GLOBAL__N_110cut_kernelEPKjPj>:
\ts_load_dwordx2 s[2:3], s[0:1], 0x0                         // 000000001000: C0060080 00000000
\ts_waitcnt lgkmcnt(0)                                       // 000000001008: BF8CC07F
\tv_mov_b32_e32 v1, 0                                        // 00000000100C: 7E020280
\ts_cbranch_scc0 2                                           // 000000001010: BF840002 <_ZN12_GLOBAL__N_110cut_kernelEPKjPj+0x1c>
\ts_endpgm                                                   // 000000001014: BF810000
\t\t...

<_Z9redo_scanILi0ELi1EEvPKtPKlS3_7MaskSel>:
\ts_load_dwordx2 s[2:3], s[0:1], 0x48                        // 000000001100: C0060080 00000048
\ts_load_dword s4, s[0:1], 0x10                              // 000000001108: C0020100 00000010
\tv_add_u32_e32 v0, s4, v0                                   // 000000001110: 68000004
\ts_endpgm                                                   // 000000001114: BF810000
\ts_nop 0                                                    // 000000001118: BF800000
\ts_nop 0                                                    // 00000000111C: BF800000

<_ZN12_GLOBAL__N_113select_kernelEiPKi>:
\ts_load_dword s2, s[0:1], 0x0                               // 000000001200: C0020080 00000000
\tv_lshlrev_b32_e32 v0, 2, v0                                // 000000001208: 24000082
\tv_add_u32_e32 v0, s2, v0                                   // 00000000120C: 68000002
\ts_endpgm                                                   // 000000001210: BF810000

<_ZN12_GLOBAL__N_123scope_fill_flags_kernelEPii>:
\ts_load_dword s3, s[0:1], 0x1c                              // 000000001300: C00200C0 0000001C
\tv_mov_b32_e32 v1, 1                                        // 000000001308: 7E020281
\ts_endpgm                                                   // 00000000130C: BF810000
"""

DIS_B = """
b.co:\tfile format elf64-amdgpu

Disassembly of section .text:

<_ZN12_GLOBAL__N_110cut_kernelEPKjPj>:
\ts_load_dwordx2 s[2:3], s[0:1], 0x0                         // 000000002000: C0060080 00000000
\ts_waitcnt lgkmcnt(0)                                       // 000000002008: BF8CC07F
\tv_mov_b32_e32 v1, 0                                        // 00000000200C: 7E020280
\ts_cbranch_scc0 2                                           // 000000002010: BF840002 <_ZN12_GLOBAL__N_110cut_kernelEPKjPj+0x1c>
\ts_endpgm                                                   // 000000002014: BF810000

<_Z9redo_scanILi0ELi1EEvPKtPKlS3_7MaskSel>:
\ts_load_dwordx2 s[2:3], s[0:1], 0x30                        // 000000002100: C0060080 00000030
\ts_load_dword s4, s[0:1], 0x10                              // 000000002108: C0020100 00000010
\tv_add_u32_e32 v0, s4, v0                                   // 000000002110: 68000004
\ts_endpgm                                                   // 000000002114: BF810000

<_ZN12_GLOBAL__N_113select_kernelEiPKi>:
\ts_load_dword s2, s[0:1], 0x0                               // 000000002200: C0020080 00000000
\tv_lshlrev_b32_e32 v0, 3, v0                                // 000000002208: 24000083
\tv_add_u32_e32 v0, s2, v0                                   // 00000000220C: 68000002
\tv_mov_b32_e32 v2, v0                                       // 000000002210: 7E040300
\ts_endpgm                                                   // 000000002214: BF810000

<_ZN12_GLOBAL__N_117fill_flags_kernelEPii>:
\ts_load_dword s3, s[0:1], 0x1c                              // 000000002300: C00200C0 0000001C
\tv_mov_b32_e32 v1, 1                                        // 000000002308: 7E020281
\ts_endpgm                                                   // 00000000230C: BF810000

<_ZN12_GLOBAL__N_110new_kernelEPi>:
\ts_endpgm                                                   // 000000002400: BF810000
"""


def notes(entries):
    """llvm-readelf --notes as it prints the metadata: an argument list nested under every kernel."""
    head = ("Displaying notes found in: .note\n  Owner                Data size \tDescription\n"
            "  AMDGPU               0x00000400\tNT_AMDGPU_METADATA (AMDGPU Metadata)\n    AMDGPU Metadata:\n        ---\n"
            "amdhsa.kernels:\n")
    body = ""
    for name, sgpr, vgpr, lds in entries:
        body += ("  - .agpr_count:     0\n    .args:\n      - .address_space:  global\n        .name:           flags\n"
                 "        .offset:         0\n        .size:           8\n        .value_kind:     global_buffer\n"
                 f"    .group_segment_fixed_size: {lds}\n    .kernarg_segment_size: 16\n    .name:           {name}\n"
                 f"    .private_segment_fixed_size: 0\n    .sgpr_count:     {sgpr}\n    .symbol:         {name}.kd\n"
                 f"    .vgpr_count:     {vgpr}\n    .wavefront_size: 64\n")
    return head + body + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\namdhsa.version:\n  - 1\n  - 2\n...\n"


NOTES_A = notes([("_ZN12_GLOBAL__N_110cut_kernelEPKjPj", 10, 4, 64), ("_Z9redo_scanILi0ELi1EEvPKtPKlS3_7MaskSel", 12, 6, 0),
                 ("_ZN12_GLOBAL__N_113select_kernelEiPKi", 8, 3, 196),
                 ("_ZN12_GLOBAL__N_123scope_fill_flags_kernelEPii", 11, 3, 0)])
NOTES_B = notes([("_ZN12_GLOBAL__N_110cut_kernelEPKjPj", 10, 4, 64), ("_Z9redo_scanILi0ELi1EEvPKtPKlS3_7MaskSel", 12, 6, 0),
                 ("_ZN12_GLOBAL__N_113select_kernelEiPKi", 9, 5, 196), ("_ZN12_GLOBAL__N_117fill_flags_kernelEPii", 11, 3, 0),
                 ("_ZN12_GLOBAL__N_110new_kernelEPi", 2, 1, 0)])


def test_parse_disassembly_strips_comments_and_padding():
    a = KD.parse_disassembly(DIS_A)
    assert list(a) == ["_ZN12_GLOBAL__N_110cut_kernelEPKjPj", "_Z9redo_scanILi0ELi1EEvPKtPKlS3_7MaskSel",
                       "_ZN12_GLOBAL__N_113select_kernelEiPKi", "_ZN12_GLOBAL__N_123scope_fill_flags_kernelEPii"]
    assert a["_ZN12_GLOBAL__N_110cut_kernelEPKjPj"] == ["s_load_dwordx2 s[2:3], s[0:1], 0x0", "s_waitcnt lgkmcnt(0)",
                                                       "v_mov_b32_e32 v1, 0", "s_cbranch_scc0 2", "s_endpgm"]
    assert a["_Z9redo_scanILi0ELi1EEvPKtPKlS3_7MaskSel"][-1] == "s_endpgm"      # the s_nop padding is gone


def test_parse_notes_reads_the_kernel_level_keys_only():
    n = KD.parse_notes(NOTES_B)
    assert len(n) == 5                       # the arguments' own .name keys made no entries
    assert n["_ZN12_GLOBAL__N_113select_kernelEiPKi"] == {"sgpr": 9, "vgpr": 5, "lds": 196, "scratch": 0}


def test_base_name():
    assert KD.base_name("_ZN12_GLOBAL__N_123scope_fill_flags_kernelEPii") == "scope_fill_flags_kernel"
    assert KD.base_name("_Z9redo_scanILi0ELi1EEvPKtPKlS3_7MaskSel") == "redo_scan"
    assert KD.base_name("plain_c_symbol") == "plain_c_symbol"


def test_compare_identical_offset_only_instruction_renamed_and_new():
    recs = KD.compare(KD.parse_disassembly(DIS_A), KD.parse_notes(NOTES_A), KD.parse_disassembly(DIS_B),
                      KD.parse_notes(NOTES_B))
    by_a = {r["a"]: r for r in recs if r["a"]}
    assert by_a["_ZN12_GLOBAL__N_110cut_kernelEPKjPj"]["status"] == "identical"
    off = by_a["_Z9redo_scanILi0ELi1EEvPKtPKlS3_7MaskSel"]
    assert off["status"] == "differs" and off["lines"] == 0          # nothing but a kernarg offset
    assert off["counts"]["a"] == off["counts"]["b"] == {"instructions": 4, "sgpr": 12, "vgpr": 6, "lds": 0, "scratch": 0}
    ins = by_a["_ZN12_GLOBAL__N_113select_kernelEiPKi"]
    assert ins["status"] == "differs" and ins["lines"] == 2          # one line replaced, one added
    assert ins["counts"]["a"] == {"instructions": 4, "sgpr": 8, "vgpr": 3, "lds": 196, "scratch": 0}
    assert ins["counts"]["b"] == {"instructions": 5, "sgpr": 9, "vgpr": 5, "lds": 196, "scratch": 0}
    ren = by_a["_ZN12_GLOBAL__N_123scope_fill_flags_kernelEPii"]
    assert ren["status"] == "renamed" and ren["b"] == "_ZN12_GLOBAL__N_117fill_flags_kernelEPii"
    assert [r for r in recs if r["status"] == "only_b"] == [{"status": "only_b", "a": None,
                                                            "b": "_ZN12_GLOBAL__N_110new_kernelEPi"}]
    assert not [r for r in recs if r["status"] == "only_a"]
    text = KD.report("canned", recs)
    assert "1 identical, 1 identical under another name, 2 differ, 0 only in A, 1 only in B" in text
    assert "differing lines, s_load offsets normalised: 0" in text and "vgpr         3 -> 5" in text


def test_renamed_and_changed_kernels_pair_by_base_name():
    a = {"_Z4scanILi0ELi1EEvPi": ["s_load_dword s2, s[0:1], 0x8", "v_mov_b32_e32 v0, 1", "s_endpgm"],
         "_Z4scanILi1ELi1EEvPi": ["s_load_dword s2, s[0:1], 0x8", "v_mov_b32_e32 v0, 2", "v_nop", "s_endpgm"]}
    b = {"_Z4scanILi1E3TagEvPi": ["s_load_dword s2, s[0:1], 0x0", "v_mov_b32_e32 v0, 2", "v_nop", "s_endpgm"],
         "_Z4scanILi0E3TagEvPi": ["s_load_dword s2, s[0:1], 0x0", "v_mov_b32_e32 v0, 1", "s_endpgm"],
         "_Z5otherPi": ["s_endpgm"]}
    recs = KD.compare(a, {}, b, {})
    pairs = {(r["a"], r["b"]): r for r in recs}
    assert pairs[("_Z4scanILi0ELi1EEvPi", "_Z4scanILi0E3TagEvPi")]["lines"] == 0
    assert pairs[("_Z4scanILi1ELi1EEvPi", "_Z4scanILi1E3TagEvPi")]["lines"] == 0
    assert pairs[(None, "_Z5otherPi")]["status"] == "only_b" and len(recs) == 3


def test_pooled_compare_follows_kernels_between_units():
    """Side A: cut_kernel in three units, move_kernel in another; side B: each once, in a new unit, move_kernel unchanged,
    scan with another instruction, one new kernel."""
    cut = ["s_load_dword s2, s[0:1], 0x0", "v_mov_b32_e32 v0, 1", "s_endpgm"]
    move = ["v_mov_b32_e32 v0, 2", "s_endpgm"]
    own = {u: {f"_Z3{u}Pi": ["v_mov_b32_e32 v0, 3", "s_endpgm"]} for u in ("aaa", "bbb", "ccc")}
    side_a = [("aaa", {"_Z10cut_kernelPi": cut, **own["aaa"]}, {"_Z10cut_kernelPi": {"vgpr": 4}}),
              ("bbb", {"_Z10cut_kernelPi": list(cut), **own["bbb"]}, {}),
              ("ccc", {"_Z10cut_kernelPi": list(cut), **own["ccc"],
                       "_Z4scanILi0EEvPi": ["s_load_dword s2, s[0:1], 0x8", "v_nop", "s_endpgm"]},
               {"_Z4scanILi0EEvPi": {"vgpr": 8}}),
              ("ddd", {"_Z11move_kernelPi": move}, {})]
    side_b = [("aaa", own["aaa"], {}), ("bbb", own["bbb"], {}),
              ("ccc", {**own["ccc"], "_Z4scanILi0EEvPi": ["s_load_dword s2, s[0:1], 0x8", "v_nop", "v_nop", "s_endpgm"]},
               {"_Z4scanILi0EEvPi": {"vgpr": 9}}),
              ("once", {"_Z10cut_kernelPi": list(cut), "_Z11move_kernelPi": list(move), "_Z10new_kernelPi": ["s_endpgm"]}, {})]
    recs, surplus = KD.compare_pooled(side_a, side_b)
    by_b = {r["b"]: r for r in recs}
    assert len(recs) == 7
    c = by_b["_Z10cut_kernelPi"]
    assert c["status"] == "identical" and c["unit"] == "once" and c["a_units"] == ["aaa", "bbb", "ccc"]
    mv = by_b["_Z11move_kernelPi"]
    assert mv["status"] == "identical" and mv["unit"] == "once" and mv["a_units"] == ["ddd"]
    sc = by_b["_Z4scanILi0EEvPi"]
    assert sc["status"] == "differs" and sc["lines"] == 1 and sc["a"] == "_Z4scanILi0EEvPi"
    assert sc["counts"] == {"a": {"instructions": 3, "vgpr": 8}, "b": {"instructions": 4, "vgpr": 9}}
    assert by_b["_Z10new_kernelPi"]["status"] == "only_b" and by_b["_Z10new_kernelPi"]["a"] is None
    assert all(by_b[f"_Z3{u}Pi"]["status"] == "identical" for u in own)
    # what A holds and B does not: two of the three copies of cut_kernel, and the scan's former instructions
    assert surplus == [{"symbol": "_Z10cut_kernelPi", "instructions": 3, "copies_a": 3, "copies_b": 1,
                        "units": ["aaa", "bbb", "ccc"]},
                       {"symbol": "_Z4scanILi0EEvPi", "instructions": 3, "copies_a": 1, "copies_b": 0, "units": ["ccc"]}]
    text = KD.report_pooled(side_a, side_b, recs, surplus)
    assert "A: 8 kernels in 4 code objects, 6 distinct" in text and "B: 7 kernels in 4 code objects, 7 distinct" in text
    assert "B against A: 5 identical, 0 identical under another name, 1 differ, 1 only in B" in text
    assert "A holds 3 copies that B does not hold, 9 instructions" in text
    assert "3 -> 1  _Z10cut_kernelPi" in text


def test_pooled_compare_finds_a_kernel_under_another_symbol():
    body = ["v_mov_b32_e32 v1, 1", "s_endpgm"]
    recs, surplus = KD.compare_pooled([("u0", {"_ZN12_GLOBAL__N_123scope_fill_flags_kernelEPii": body}, {})],
                                      [("u1", {"_ZN12_GLOBAL__N_117fill_flags_kernelEPii": list(body)}, {})])
    assert [(r["status"], r["a"], r["a_units"]) for r in recs] == [
        ("renamed", "_ZN12_GLOBAL__N_123scope_fill_flags_kernelEPii", ["u0"])]
    assert [(s["symbol"], s["copies_a"], s["copies_b"]) for s in surplus] == [
        ("_ZN12_GLOBAL__N_123scope_fill_flags_kernelEPii", 1, 0)]
