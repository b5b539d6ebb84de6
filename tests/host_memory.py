"""An ``EmbeddingMemory`` without a device: the host-side rules of its methods run, and every call that reaches the
library goes to the stand-in given here (by default one that fails the test; ``SizingLibrary`` answers the sizing
calls only)."""
import torch


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were checked")


class SizingLibrary:
    """Every ``vm_*_workspace_bytes`` entry: 1,000 bytes plus 64 per unit of its arguments.  Nothing else exists."""

    def __getattr__(self, name):
        if not name.endswith("_workspace_bytes"):
            raise AssertionError(f"library call {name}: the owner rule only sizes")
        return lambda handle, *args: 1000 + 64 * sum(int(a) for a in args)


def owner_rule_holds(kind, prepare):
    """The owner rule on a search scratch sized by (Q, k) - ``kind``: its class in vidmem.memory, ``prepare``: the
    memory's method for it -, against the sizing stand-in: kept while it fits, replaced to grow and never resized, a
    caller's scratch refused when too small and used when it fits.  -> the memory, which has run no search."""
    import pytest
    from vidmem import memory as M
    kind = getattr(M, kind)
    mem = host_memory(capacity=16, library=SizingLibrary())
    first = getattr(mem, prepare)(4, 10)
    assert isinstance(first, kind) and first.fits(mem, 4, 10)
    assert first.ws.numel() == 1000 + 64 * 14 and first.flags.dtype == torch.int32 and (first.flags == 0).all()
    assert set(scratch_buffers(first)) == {"ws", "flags"}
    before = scratch_buffers(first)
    assert getattr(mem, prepare)(4, 10) is first and mem._resolve(kind, None, 2, 5) is first
    grown = getattr(mem, prepare)(64, 32)
    assert grown is not first and grown.fits(mem, 64, 32) and scratch_buffers(first) == before   # replaced, never resized
    with pytest.raises(ValueError, match="too small"):
        mem._resolve(kind, kind.for_(mem, 4, 10), 64, 32)
    theirs = kind.for_(mem, 64, 32)
    assert mem._resolve(kind, theirs, 64, 32) is theirs
    return mem


def scratch_buffers(scratch):
    """name -> (address, elements) of every tensor a scratch object owns."""
    return {name: (t.data_ptr(), t.numel()) for name, t in vars(scratch).items() if isinstance(t, torch.Tensor)}


def host_memory(grouped=False, tagged=False, dim=128, dtype="f16", capacity=16, library=None):
    from vidmem.memory import EmbeddingMemory, _torch_dtype
    mem = EmbeddingMemory.__new__(EmbeddingMemory)      # host rules only: no device handle
    mem.grouped, mem.tagged, mem.capacity, mem.ring = grouped, tagged, capacity, False
    mem.dim, mem.dtype_name, mem.dtype = dim, dtype, _torch_dtype(dtype)
    mem.L = mem.ctx = library if library is not None else NoLibrary()
    mem.handle = None
    mem.device = torch.device("cpu")
    mem._init_scratch()
    return mem
