"""CPU: the C-ABI library builds for gfx950, loads, exports every symbol include/vidmem.h declares, and fails loudly
without a GPU (no compute call is made here)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vidmem.h")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from vidmem import _lib
    return _lib


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vm_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported(built):
    L = built.lib()
    names = declared_symbols()
    assert len(names) >= 28
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/vidmem.h but not exported by libvidmem.so"
    assert sorted(built.SYMBOLS) == names, "python binding table and header disagree"


def test_exports_are_plain_c(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for n in declared_symbols():
        assert n in exported  # unmangled extern "C" names


def test_gfx950_code_object_is_embedded(built):
    data = open(built.LIB_PATH, "rb").read()
    assert b"gfx950" in data and b"gfx942" not in data and b"sm_" not in data


def test_release_library_reads_no_environment(built):
    """The developer A/B switches (csrc/vm_common.h VM_DEV_ENV) are compiled to their defaults in the release library: no
    VIDMEM_* name and no getenv import may be left in it - a stray variable in a deployment's environment must not be
    able to change which kernel produces product results."""
    data = open(built.LIB_PATH, "rb").read()
    assert b"VIDMEM_" not in data
    und = subprocess.check_output(["nm", "-D", "--undefined-only", built.LIB_PATH], text=True)
    assert "getenv" not in und


def test_no_gpu_means_loud_failure(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(built.VidmemError) as e:
        built.Context(0)
    assert e.value.code == built.VM_ERR_NO_DEVICE
    h = ctypes.c_void_p()
    assert built.lib().vm_init(0, ctypes.byref(h)) == built.VM_ERR_NO_DEVICE
    assert built.lib().vm_abi_version() == 4


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "real-time-brain-inspired-video-memory_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("the oracle", "").replace("oracle's", "").replace(
                    "as the oracle", "").replace("The oracle", "") or "import" not in src.split("oracle")[0][-40:], f
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), f


def test_gemm_tile_guard(tmp_path):
    """csrc/gemm_guard.h: the 256 x 256 GEMM kernels address a tile through 32-bit byte offsets inside a per-tile buffer
    descriptor; shapes whose tile would not fit below 2^31 bytes must be refused (they take the 128 x 128 kernel with
    64-bit pointers).  Host-only: compiled with g++, no HIP."""
    src = tmp_path / "guard.cpp"
    src.write_text(r'''
#include "gemm_guard.h"
#include <cstdio>
int main() {
    struct { long long K, ldx; bool want; } c[] = {
        {768, 768, true}, {3072, 3072, true}, {4096, 4096, true},
        {768, 197LL * 768, true},                 // CLS rows addressed in place: row stride = one frame of tokens
        {1024, 577LL * 1024, true},
        {64, (1LL << 23) + 64, false},            // 255 rows x 16 MB stride: past 2^31
        {(1LL << 22), (1LL << 22), false},        // 256 weight rows x 8 MB
        {768, 512, false}, {0, 768, false},       // stride below the row length / empty rows
    };
    int bad = 0;
    for (auto &t : c) if (vm_gemm256_tile_addressable(t.K, t.ldx) != t.want) { std::printf("K=%lld ldx=%lld\n", t.K, t.ldx); ++bad; }
    // the limit itself: 255 * ldx + K elements of 2 bytes must stay below 2^31 bytes
    long long ldx = ((1LL << 30) - 768) / 255;
    if (!vm_gemm256_tile_addressable(768, ldx)) ++bad;
    if (vm_gemm256_tile_addressable(768, ldx + 4)) ++bad;
    return bad;
}
''')
    exe = tmp_path / "guard"
    inc = os.path.join(ROOT, "real-time-brain-inspired-video-memory_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", inc, str(src), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def test_gemm_leaves_room_for_the_layernorm(built, tmp_path):
    """The two-stream encoder schedule (csrc/encoder.hip) rests on a register budget: a SIMD has 512 vector registers,
    allocated in steps of 8; the persistent GEMM runs two waves per SIMD, the low-register LayerNorm of the other stream
    is admitted beside them only if 2 x GEMM + LayerNorm <= 512.  Round 4 lost that silently (GEMM 221 -> 227 registers =
    232 allocated, LayerNorm 58 = 64: 528) and got it back; this reads the counts out of the BUILT library's gfx950 code
    objects so that it cannot happen silently again.  FC1's instantiation (GELU16: the table lookups in flight) is
    known to be above the step and exempt."""
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("llvm tools of the ROCm image not found")
    import shutil
    so = str(tmp_path / "libvidmem.so")
    shutil.copy(built.LIB_PATH, so)
    subprocess.check_call([objdump, "--offloading", so], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=str(tmp_path))
    counts = {}
    for f in os.listdir(tmp_path):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([readelf, "--notes", str(tmp_path / f)], capture_output=True, text=True).stdout
        name = None
        for line in notes.splitlines():
            line = line.strip()
            if line.startswith(".name:"):
                name = line.split(":", 1)[1].strip()
            elif line.startswith(".vgpr_count:") and name:
                counts[name] = int(line.split(":", 1)[1])
    alloc = lambda n: (n + 7) // 8 * 8
    gemm = {k: v for k, v in counts.items() if "gemm256p_kernel" in k}
    ln = {k: v for k, v in counts.items() if "resid_layernorm_lowreg_kernel" in k}
    assert len(gemm) >= 8 and len(ln) >= 4, (len(gemm), len(ln), len(counts))
    ln_alloc = max(alloc(v) for v in ln.values())
    over = []
    for k, v in gemm.items():
        # template arguments <dtype, epilogue, ablation>
        m = re.search(r"gemm256p_kernelILi(\d)ELi(\d)ELi(\d+)E", k)
        assert m, k
        if m.group(2) not in ("0", "2", "5"):   # vm_encode's 16-bit epilogues: STORE16, QGELU16, DELTA16 (GELU16 exempt;
            continue                            # the fp32 epilogues 3 / 4 are not launched by the encoder)
        if 2 * alloc(v) + ln_alloc > 512:
            over.append((k, v))
    assert not over, f"GEMM instantiations that no longer leave {ln_alloc} registers per SIMD: {over}"


def test_no_kernel_is_compiled_twice(built, tmp_path):
    """Every kernel symbol is defined in one gfx950 code object of libvidmem.so, the whole library over.  A kernel in a
    header's anonymous namespace is compiled again by every translation unit that includes the header: five copies of
    the key-image select stage and two of the grouped table and compaction were in the library that way,
    and a per-kernel profile of one stage was spread over as many symbols.  Kernels that are identical under different
    symbols inside one unit are not this test's business."""
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("llvm tools of the ROCm image not found")
    import shutil
    so = str(tmp_path / "libvidmem.so")
    shutil.copy(built.LIB_PATH, so)
    subprocess.check_call([objdump, "--offloading", so], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=str(tmp_path))
    units = {}
    for f in sorted(os.listdir(tmp_path)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([readelf, "--notes", str(tmp_path / f)], capture_output=True, text=True).stdout
        for sym in re.findall(r"^\s*\.symbol:\s*(\S+)\.kd\s*$", notes, flags=re.M):   # one per kernel, none per argument
            units.setdefault(sym, []).append(f)
    n_units = len({f for fs in units.values() for f in fs})
    assert n_units >= 20 and len(units) >= 300, (n_units, len(units))   # the whole library, the encoder's units included
    twice = {s: fs for s, fs in units.items() if len(fs) > 1}
    assert not twice, f"kernels defined in more than one code object: {twice}"
