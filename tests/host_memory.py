"""An ``EmbeddingMemory`` without a device: the host-side rules of its methods run, and every call that reaches the
library goes to the stand-in given here (by default one that fails the test)."""
import torch


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were checked")


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
