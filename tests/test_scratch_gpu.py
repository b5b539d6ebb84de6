"""GPU: a captured ``topk_scoped`` / ``topk_grouped`` / ``topk_grouped_scoped`` on a caller-owned scratch survives a
later, larger eager call on the same memory.

The hazard: a hipGraph bakes in the addresses of the workspace and flag buffers it was captured with.  The memory's own
scratch is replaced when a larger call needs more, so a graph must not depend on it; ``scratch=`` gives the capture
buffers that nobody else touches.  The smallest shape that reaches it: 256 clustered rows in a memory of 2,048, a capture
at (Q, k) = (4, 10), one eager call at (64, 32) that makes the memory's own scratch grow, then a replay with new queries
and windows.  Bar: rows and fp64 score bits equal to the host oracles of the neighbouring test files, for the replay and
for the eager call, whose outputs the replay must leave alone."""
import time

import numpy as np
import pytest
import torch

from tests import group_ref as G
from tests import group_scope_ref as GS
from tests import scope_ref as S
from tests.support import MS, bits, clustered, make_tag, queries_near, scope_of

pytestmark = pytest.mark.gpu

D, ROWS, CAPACITY = 768, 256, 2048
CAPTURED, EAGER = (4, 10), (64, 32)
SEARCHES = {    # method -> (prepare_*, last_*_flags, takes a scope)
    "topk_scoped": ("prepare_topk_scoped", "last_scope_flags", True),
    "topk_grouped": ("prepare_topk_grouped", "last_group_flags", False),
    "topk_grouped_scoped": ("prepare_topk_grouped_scoped", "last_group_scope_flags", True),
}
WINDOWS = [[scope_of(0), scope_of(1, MS * 10, MS * 100), scope_of(0, MS * 5, MS * 60), (7, 3)],
           [scope_of(1), scope_of(0, MS * 20, MS * 90), (S.INT64_MIN, S.INT64_MAX), scope_of(2)]]


def finish(step, seconds=20.0):
    """Every step has its own time limit: the work queued so far completes within it, or the whole session ends there
    (after a hang nothing more may start on the GPU)."""
    done = torch.cuda.Event()
    done.record()
    deadline = time.monotonic() + seconds
    while not done.query():
        if time.monotonic() > deadline:
            pytest.exit(f"{step}: the GPU did not finish within {seconds} s", returncode=1)
        time.sleep(0)       # steps take milliseconds: yield the core, do not wait


def oracle(name, mem, q, k, scopes):
    """-> the arrays in the order the search returns them: scores, rows (, keys)."""
    base, host_rows = mem.rows_host()
    if name == "topk_scoped":
        r, s = S.scoped_topk(bits(q), host_rows, mem.tags_host(), scopes, k, dtype="f16", base=base)
        return s, r
    if name == "topk_grouped":
        r, s, kk = G.grouped_topk(bits(q), host_rows, mem.group_keys_host(), k, dtype="f16", base=base)
    else:
        r, s, kk = GS.group_scoped_topk(bits(q), host_rows, mem.group_keys_host(), mem.tags_host(), scopes, k,
                                        dtype="f16", base=base)
    return s, r, kk


def same(got, want):
    return len(got) == len(want) and all(
        np.array_equal(g.cpu().numpy().view(np.int64), np.ascontiguousarray(w).view(np.int64)) for g, w in zip(got, want))


@pytest.mark.parametrize("name", list(SEARCHES))
def test_captured_search_on_its_own_scratch_survives_a_larger_eager_call(name):
    from vidmem.memory import EmbeddingMemory
    prepare, last, scoped = SEARCHES[name]
    rows, _ = clustered([4] * (ROWS // 4), D, "f16", seed=61)
    i = torch.arange(ROWS, device="cuda")
    mem = EmbeddingMemory(CAPACITY, D, "f16", grouped=True, tagged=True)
    mem.append(rows, group=i // 4, tag=((i // 128) << 40) | ((i % 128) * MS))
    assert make_tag(1, 5 * MS) == int(mem.tags_host()[133])
    search = getattr(mem, name)
    (Q, k), (Qe, ke) = CAPTURED, EAGER

    # 1. the memory's own scratch (and its counter) exist at the captured size; the capture gets buffers of its own
    own = getattr(mem, prepare)(Q, k)
    theirs = type(own).for_(mem, Q, k)
    own_ws, their_ws = own.ws.data_ptr(), theirs.ws.data_ptr()
    q = queries_near(rows, Q, 6, "f16")
    scope = torch.tensor(WINDOWS[0], dtype=torch.int64, device="cuda")
    finish("setup")

    # 2. capture one call on a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = search(q, k, scope, scratch=theirs) if scoped else search(q, k, scratch=theirs)
    torch.cuda.current_stream().wait_stream(side)
    finish("capture")
    assert getattr(mem, last) is theirs.flags

    # 3. one larger eager call: the memory's own scratch must grow, by replacement
    qe = queries_near(rows, Qe, 7, "f16")
    scopes_e = [WINDOWS[j % 2][j % 4] for j in range(Qe)]
    eager = search(qe, ke, scopes_e) if scoped else search(qe, ke)
    finish("eager call")
    grown = getattr(mem, prepare)(Qe, ke)
    assert grown is not own and grown is not theirs and grown.fits(mem, Qe, ke) and not own.fits(mem, Qe, ke)
    assert getattr(mem, last) is grown.flags
    assert (own.ws.data_ptr(), theirs.ws.data_ptr()) == (own_ws, their_ws) and theirs.fits(mem, Q, k)
    kept = [t.clone() for t in eager]

    # 4. new queries and windows in place, then the replay
    q.copy_(queries_near(rows, Q, 10, "f16"))
    scope.copy_(torch.tensor(WINDOWS[1], dtype=torch.int64))
    graph.replay()
    finish("replay")

    # 5. the replay answered the new queries, and left the eager call's outputs intact
    assert same(out, oracle(name, mem, q, k, WINDOWS[1]))
    assert all(torch.equal(a, b) for a, b in zip(eager, kept))
    assert same(eager, oracle(name, mem, qe, ke, scopes_e))
    assert getattr(mem, last) is grown.flags
