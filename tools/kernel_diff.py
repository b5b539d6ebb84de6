"""Per-kernel comparison of the gfx950 device code of two builds (the check that a refactor left the
kernels it only meant to move as they were).

  python tools/kernel_diff.py A/csrc B/csrc --files topk_scope topk_mask ... [--names parent new] [--out report.txt]
  python tools/kernel_diff.py A/libvidmem.so B/libvidmem.so [--out report.txt]

Two ``csrc`` directories: every named ``.hip`` (default: all that both hold) is compiled on each side with the Makefile's
flags plus ``--offload-device-only --no-gpu-bundle-output``.  Two built libraries: the gfx950 code object of every
translation unit is taken out of ``.hip_fatbin``, in link order.  Either way each code object is read with ``llvm-objdump
-d --no-show-raw-insn --no-leading-addr`` and ``llvm-readelf --notes`` and the two sides are compared per kernel symbol:

  identical            the same instructions under the same symbol
  identical (renamed)  the same instructions under another symbol (a kernel that moved or whose template arguments changed)
  differs              with instruction count, SGPRs, VGPRs, LDS bytes and scratch bytes of both sides, and the number of
                       differing lines once the kernarg offsets of ``s_load_*`` are normalised (0: offsets only)
  only in A / only in B

A kernel only in A and one only in B that differ are reported as one differing pair when they share a base name (the
function's name without namespace, template arguments and signature); among several, the pairs with the fewest differing
lines.  The tool only compares: it looks for no particular instruction.

``--pooled``: for two builds whose kernels moved between translation units (the sides may hold different numbers of code
objects).  Every kernel of B, whatever unit holds it, is looked up among all kernels of A: identical under its symbol,
identical under another, differing from its closest A kernel of the same base name, or only in B.  Then, per (symbol,
instructions), the copies A holds and B no longer does.

parse_disassembly, parse_notes, compare and compare_pooled work on text and have no subprocess in them (tests/test_kernel_diff_cpu.py).
"""
import argparse
import difflib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
# csrc/Makefile's CXXFLAGS, then the two flags that leave a plain device ELF
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
         "--offload-device-only", "--no-gpu-bundle-output"]


# ---- text in, comparison out -----------------------------------------------------------------------------------------
def parse_disassembly(text):
    """{symbol: [instruction, ...]} of an ``llvm-objdump -d`` listing: the ``//`` encoding comments (which also carry the
    branch targets' symbol names) and the padding after the last instruction dropped, white space squeezed."""
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(?:[0-9a-fA-F]+\s+)?<([^>]+)>:\s*$", line)
        if m:
            cur = kernels.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        ins = " ".join(line.split("//", 1)[0].split())
        if ins and ins != "...":
            cur.append(ins)
    for ins in kernels.values():
        while ins and ins[-1].startswith(("s_nop", "s_code_end")):
            ins.pop()
    return kernels


_NOTE_KEYS = {".sgpr_count": "sgpr", ".vgpr_count": "vgpr", ".group_segment_fixed_size": "lds",
              ".private_segment_fixed_size": "scratch"}


def parse_notes(text):
    """{symbol: {"sgpr", "vgpr", "lds", "scratch"}} of ``llvm-readelf --notes``: the entries of amdhsa.kernels."""
    out, cur, indent = {}, None, None
    for line in text.splitlines():
        if line.strip() == "amdhsa.kernels:":
            indent = None
            cur = {}
            continue
        if cur is None:
            continue
        m = re.match(r"^(\s*)(- )?(\.\w+):\s*(.*)$", line)
        if not m:
            if line and not line[0].isspace():   # the next top-level key of the metadata ends the list
                cur = None
            continue
        lead, dash, key, val = m.groups()
        if dash and (indent is None or len(lead) == indent):
            indent = len(lead)
            cur = {}
        elif len(lead) != (indent or 0) + 2:
            continue                             # a key of an argument, nested deeper
        if key == ".name":
            out[val.strip()] = cur
        elif key in _NOTE_KEYS:
            cur[_NOTE_KEYS[key]] = int(val)
    return {k: v for k, v in out.items() if v}


def base_name(symbol):
    """The function's own name inside an Itanium-mangled symbol (no namespace, template arguments, signature)."""
    m = re.match(r"^_Z(N?)", symbol)
    if not m:
        return symbol
    pos, name = m.end(), None
    while True:
        n = re.match(r"\d+", symbol[pos:])
        if not n:
            break
        pos += n.end()
        ident, pos = symbol[pos:pos + int(n.group())], pos + int(n.group())
        if not ident.startswith("_GLOBAL__N"):
            name = ident
            break
    return name or symbol


def normalise(instructions):
    """The kernarg offset of every s_load_* replaced by a placeholder: an argument list that changed moves them."""
    return [re.sub(r",\s*(0x[0-9a-fA-F]+|\d+)$", ", OFF", i) if i.startswith("s_load_") else i for i in instructions]


def differing_lines(a, b):
    """Lines outside the common subsequence of two (normalised) listings: per replaced block, the longer side."""
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")


def compare(dis_a, notes_a, dis_b, notes_b):
    """Records, one per kernel (or pair of kernels): dicts with "status" ("identical", "renamed", "differs", "only_a",
    "only_b"), "a" / "b" (symbol or None) and, for "differs", "counts" (per side: instructions, sgpr, vgpr, lds,
    scratch) and "lines" (differing lines after normalise)."""
    recs = []
    only_a = [s for s in dis_a if s not in dis_b]
    only_b = [s for s in dis_b if s not in dis_a]

    def differs(sa, sb):
        counts = {side: dict(instructions=len(d[s]), **n.get(s, {}))
                  for side, d, n, s in (("a", dis_a, notes_a, sa), ("b", dis_b, notes_b, sb))}
        return {"status": "differs", "a": sa, "b": sb, "counts": counts,
                "lines": differing_lines(normalise(dis_a[sa]), normalise(dis_b[sb]))}

    for s in dis_a:
        if s in dis_b:
            recs.append({"status": "identical", "a": s, "b": s} if dis_a[s] == dis_b[s] else differs(s, s))
    for sa in list(only_a):   # the same instructions under another name
        sb = next((s for s in only_b if dis_b[s] == dis_a[sa]), None)
        if sb is not None:
            recs.append({"status": "renamed", "a": sa, "b": sb})
            only_a.remove(sa)
            only_b.remove(sb)
    pairs = sorted((differs(sa, sb) for sa in only_a for sb in only_b if base_name(sa) == base_name(sb)),
                   key=lambda r: r["lines"])
    for r in pairs:           # other instructions under another name: closest pairs of one base name first
        if r["a"] in only_a and r["b"] in only_b:
            recs.append(r)
            only_a.remove(r["a"])
            only_b.remove(r["b"])
    recs += [{"status": "only_a", "a": s, "b": None} for s in only_a]
    recs += [{"status": "only_b", "a": None, "b": s} for s in only_b]
    return recs


def report(unit, recs):
    """The records of one code object as text."""
    n = {k: sum(r["status"] == k for r in recs) for k in ("identical", "renamed", "differs", "only_a", "only_b")}
    lines = [f"== {unit}: {n['identical']} identical, {n['renamed']} identical under another name, "
             f"{n['differs']} differ, {n['only_a']} only in A, {n['only_b']} only in B"]
    for r in recs:
        if r["status"] == "identical":
            lines.append(f"  identical            {r['a']}")
        elif r["status"] == "renamed":
            lines.append(f"  identical (renamed)  {r['a']}\n                    -> {r['b']}")
        elif r["status"] == "differs":
            lines.append(f"  differs              {r['a']}" + ("" if r["a"] == r["b"] else f"\n                    -> {r['b']}"))
            for key in ("instructions", "sgpr", "vgpr", "lds", "scratch"):
                lines.append(f"      {key:<13}{r['counts']['a'].get(key, '?')} -> {r['counts']['b'].get(key, '?')}")
            lines.append(f"      differing lines, s_load offsets normalised: {r['lines']}")
        else:
            lines.append(f"  only in {'A' if r['status'] == 'only_a' else 'B'}            {r['a'] or r['b']}")
    return "\n".join(lines)


def compare_pooled(side_a, side_b):
    """The comparison for two builds whose kernels moved between translation units: every kernel of a side is pooled,
    whatever unit holds it.  side_*: [(unit, disassembly, notes)].  Returns (recs, surplus).  recs, one per kernel of B
    and unit that holds it: "status" ("identical": a kernel of A has these instructions under this symbol; "renamed":
    under another symbol; "differs": from its closest A kernel of the same base name, with "counts" and "lines" as in
    compare; "only_b"), "unit", "b", "a" and "a_units".  surplus, one per (symbol, instructions) that A holds more often
    than B: "symbol", "instructions", "copies_a", "copies_b", "units" (A's)."""
    by_sym, by_body, copies_b = {}, {}, {}
    for unit, dis, notes in side_a:
        for s, ins in dis.items():
            by_sym.setdefault(s, []).append((unit, ins, notes.get(s, {})))
            by_body.setdefault(tuple(ins), []).append((unit, s))
    recs = []
    for unit, dis, notes in side_b:
        for s, ins in dis.items():
            copies_b[s, tuple(ins)] = copies_b.get((s, tuple(ins)), 0) + 1
            rec = {"unit": unit, "b": s, "a": None, "a_units": []}
            same = [u for u, i, _ in by_sym.get(s, []) if i == ins]
            if same:
                rec.update(status="identical", a=s, a_units=same)
            elif tuple(ins) in by_body:
                sa = by_body[tuple(ins)][0][1]
                rec.update(status="renamed", a=sa, a_units=[u for u, x in by_body[tuple(ins)] if x == sa])
            else:
                near = [(differing_lines(normalise(ia), normalise(ins)), sa, ua, ia, na)
                        for sa, held in by_sym.items() if base_name(sa) == base_name(s) for ua, ia, na in held]
                if near:
                    lines, sa, ua, ia, na = min(near, key=lambda t: t[0])
                    rec.update(status="differs", a=sa, a_units=[ua], lines=lines,
                               counts={"a": dict(instructions=len(ia), **na),
                                       "b": dict(instructions=len(ins), **notes.get(s, {}))})
                else:
                    rec["status"] = "only_b"
            recs.append(rec)
    surplus = []
    for s, held in by_sym.items():
        for body in dict.fromkeys(tuple(i) for _, i, _ in held):
            units = [u for u, i, _ in held if tuple(i) == body]
            if len(units) > copies_b.get((s, body), 0):
                surplus.append({"symbol": s, "instructions": len(body), "copies_a": len(units),
                                "copies_b": copies_b.get((s, body), 0), "units": units})
    return recs, surplus


def report_pooled(side_a, side_b, recs, surplus):
    """The pooled comparison as text."""
    def held(side):
        bodies = [(s, tuple(i)) for _, dis, _ in side for s, i in dis.items()]
        return f"{len(bodies)} kernels in {len(side)} code objects, {len(set(bodies))} distinct"
    n = {k: sum(r["status"] == k for r in recs) for k in ("identical", "renamed", "differs", "only_b")}
    lines = [f"== pooled\nA: {held(side_a)}\nB: {held(side_b)}",
             f"B against A: {n['identical']} identical, {n['renamed']} identical under another name, "
             f"{n['differs']} differ, {n['only_b']} only in B"]
    for r in recs:
        src = f"  [{r['unit']} <- A: {', '.join(r['a_units'])}]"
        if r["status"] == "identical":
            lines.append(f"  identical            {r['b']}{src}")
        elif r["status"] == "renamed":
            lines.append(f"  identical (renamed)  {r['a']}\n                    -> {r['b']}{src}")
        elif r["status"] == "differs":
            lines.append(f"  differs              {r['a']}" + ("" if r["a"] == r["b"] else f"\n                    -> {r['b']}")
                         + src)
            for key in ("instructions", "sgpr", "vgpr", "lds", "scratch"):
                lines.append(f"      {key:<13}{r['counts']['a'].get(key, '?')} -> {r['counts']['b'].get(key, '?')}")
            lines.append(f"      differing lines, s_load offsets normalised: {r['lines']}")
        else:
            lines.append(f"  only in B            {r['b']}  [{r['unit']}]")
    gone = sum(s["copies_a"] - s["copies_b"] for s in surplus)
    ins = sum((s["copies_a"] - s["copies_b"]) * s["instructions"] for s in surplus)
    lines.append(f"A holds {gone} copies that B does not hold, {ins} instructions")
    for s in surplus:
        lines.append(f"  {s['copies_a']} -> {s['copies_b']}  {s['symbol']}  ({s['instructions']} instructions; A: "
                     f"{', '.join(s['units'])})")
    return "\n".join(lines)


# ---- the subprocess half ---------------------------------------------------------------------------------------------
def read_code_object(path):
    dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr",
                                   path], text=True)
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", path], text=True)
    return parse_disassembly(dis), parse_notes(notes)


def compile_device(src, out):
    subprocess.check_call([HIPCC, *FLAGS, "-c", src, "-o", out])


def library_code_objects(lib, tmp, tag):
    """The gfx950 ELF of every offload bundle in the library's .hip_fatbin, in order: [(unit name, path)]."""
    fat = os.path.join(tmp, f"{tag}.fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib,
                           os.path.join(tmp, f"{tag}.discard")])
    data, magic, out = open(fat, "rb").read(), b"__CLANG_OFFLOAD_BUNDLE__", []
    starts = [m.start() for m in re.finditer(re.escape(magic), data)]
    for i, s in enumerate(starts):
        (count,), pos = struct.unpack_from("<Q", data, s + len(magic)), s + len(magic) + 8
        for _ in range(count):
            off, size, tlen = struct.unpack_from("<QQQ", data, pos)
            triple, pos = data[pos + 24:pos + 24 + tlen].decode(), pos + 24 + tlen
            if ARCH in triple and size:
                path = os.path.join(tmp, f"{tag}_{i:02d}.co")
                with open(path, "wb") as f:
                    f.write(data[s + off:s + off + size])
                out.append((f"unit {i:02d}", path))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a", help="csrc directory or built library of side A (the parent)")
    ap.add_argument("b", help="the same of side B")
    ap.add_argument("--files", nargs="*", default=None, help="with directories: the .hip files to compare, without suffix")
    ap.add_argument("--names", nargs=2, default=None, metavar=("A", "B"), help="what the report calls the two sides")
    ap.add_argument("--pooled", action="store_true",
                    help="compare all kernels of A with all kernels of B, whatever unit holds them (kernels that moved)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        if os.path.isdir(args.a) != os.path.isdir(args.b):
            sys.exit("kernel_diff: give two directories or two libraries")
        if os.path.isdir(args.a):
            names = args.files or sorted(f[:-4] for f in os.listdir(args.a)
                                         if f.endswith(".hip") and os.path.exists(os.path.join(args.b, f)))
            units = []
            for name in names:
                pa, pb = os.path.join(tmp, f"a_{name}.co"), os.path.join(tmp, f"b_{name}.co")
                compile_device(os.path.join(args.a, name + ".hip"), pa)
                compile_device(os.path.join(args.b, name + ".hip"), pb)
                units.append((name + ".hip", pa, pb))
        else:
            ua, ub = library_code_objects(args.a, tmp, "a"), library_code_objects(args.b, tmp, "b")
            if args.pooled:
                units = []
            elif len(ua) != len(ub):
                sys.exit(f"kernel_diff: {len(ua)} code objects in A, {len(ub)} in B (--pooled compares such builds)")
            else:
                units = [(na, pa, pb) for (na, pa), (_, pb) in zip(ua, ub)]
        na, nb = args.names or (args.a, args.b)
        text = [f"A = {na}\nB = {nb}"]
        if args.pooled:
            if os.path.isdir(args.a):
                ua, ub = [(n, pa) for n, pa, _ in units], [(n, pb) for n, _, pb in units]
            side_a = [(n, *read_code_object(p)) for n, p in ua]
            side_b = [(n, *read_code_object(p)) for n, p in ub]
            text.append(report_pooled(side_a, side_b, *compare_pooled(side_a, side_b)))
            units = []
        for name, pa, pb in units:
            text.append(report(name, compare(*read_code_object(pa), *read_code_object(pb))))
    text = "\n\n".join(text) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
