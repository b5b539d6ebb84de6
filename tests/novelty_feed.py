"""A repetitive frame feed for the novelty tests: every source frame (random colour blocks) is shown 1-4 times in a row,
each showing with its own +-1 of pixel noise."""
import numpy as np


def feed(seed: int, n_src: int, H: int, W: int, block: int = 32):
    """-> (frames uint8 [n, H, W, 3], owner int [n]: the source frame of every frame)."""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 256, size=(n_src, H // block, W // block, 3), dtype=np.uint8)
    src = np.kron(blocks, np.ones((1, block, block, 1), np.uint8))
    frames, owner = [], []
    for i in range(n_src):
        for _ in range(int(rng.integers(1, 5))):
            noise = rng.integers(-1, 2, size=src[i].shape)
            frames.append(np.clip(src[i].astype(np.int16) + noise, 0, 255).astype(np.uint8))
            owner.append(i)
    return np.stack(frames), np.array(owner)


def threshold_between(scores: np.ndarray, owner: np.ndarray) -> float:
    """A threshold picked from the reference's own score matrix of the feed's embeddings: halfway between the lowest
    score of two showings of one source frame and the highest score of two different source frames, which must be
    separated."""
    same = owner[:, None] == owner[None, :]
    off = ~np.eye(owner.size, dtype=bool)
    lo_rep = scores[same & off].min()
    hi_dist = scores[~same].max()
    print(f"repeated-frame scores >= {lo_rep!r}, distinct-frame scores <= {hi_dist!r}")
    assert hi_dist < lo_rep, (hi_dist, lo_rep)
    return float((lo_rep + hi_dist) / 2.0)
