"""CPU: the stage tests' shim (tests/native/stage_shim.cpp -> libvidmem_stages.so) builds and loads without a GPU, exports
its wrappers, links against the release library instead of carrying kernels of its own, and leaves libvidmem.so mapped
once in the process.  A missing shim fails here; nothing skips."""
import os
import subprocess

import pytest

import tests.stage_lib as SL


@pytest.fixture(scope="module")
def built():
    # the stages target alone: libvidmem.so is its prerequisite, so a fresh tree builds the release library first and an
    # up-to-date one is left alone (nothing relinks a library this process may already have mapped)
    import __graft_entry__ as g
    subprocess.check_call(["make", "-s", "-C", os.path.join(g.PKG, "csrc"), "stages"])
    from vidmem import _lib
    return _lib


def test_shim_builds_loads_and_exports_the_wrappers(built):
    assert os.path.exists(SL.shim_path()), "build() did not produce libvidmem_stages.so beside libvidmem.so"
    S = SL.stages()
    for name in SL.WRAPPERS:
        assert hasattr(S, name), f"{name} is not exported by the shim"
    out = subprocess.check_output(["nm", "-D", "--defined-only", SL.shim_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(SL.WRAPPERS) <= exported
    assert not any(n.startswith("vm_") for n in exported), "the shim must not define or re-export vm_* symbols"


def test_shim_links_against_the_release_library(built):
    dyn = subprocess.check_output(["readelf", "-d", SL.shim_path()], text=True)
    assert "Shared library: [libvidmem.so]" in dyn, "the shim does not name libvidmem.so as a dependency"
    assert "$ORIGIN" in dyn, "the shim's run path does not start at its own directory"
    data = open(SL.shim_path(), "rb").read()
    assert b"gemm256p_kernel" not in data and b"resid_layernorm_kernel" not in data, "kernels were compiled into the shim"
    und = subprocess.check_output(["nm", "-D", "--undefined-only", SL.shim_path()], text=True)
    for launcher in ("vm_gemm", "vm_attention", "vm_resid_layernorm", "vm_embed", "vm_pool", "vm_text_embed",
                     "vm_gemm_set_variant"):
        assert launcher in und, f"the shim does not import {launcher} from the release library"


def test_release_library_is_mapped_once(built):
    built.lib()
    SL.stages()
    assert SL.mapped_copies("libvidmem.so") == 1, "libvidmem.so is mapped from two files: the shim found another copy"
    assert SL.mapped_copies("libvidmem_stages.so") == 1
    assert SL.mapped_copies("libvidmem_dev.so") == 0, "the developer build must not come in with the shim"


def test_release_exports_are_unchanged_by_the_shim(built):
    """The shim adds nothing to libvidmem.so: its extern "C" export table is still exactly include/vidmem.h."""
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.LIB_PATH], text=True)
    plain_c = sorted(l.split()[-1] for l in out.splitlines() if " T " in l and not l.split()[-1].startswith("_Z"))
    assert [n for n in plain_c if n.startswith("vmt_")] == []
    assert sorted(n for n in plain_c if n.startswith("vm_")) == sorted(built.SYMBOLS)
