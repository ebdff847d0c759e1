"""Synthetic verification sets for the fixture (tools/make_golden.py), the tests and tools/verification_bench.py.

FROZEN: tests/golden/verification.npz was captured from the reference on exactly these inputs.  Any change to the draws below (their
order, shapes or distributions) invalidates the fixture; tests/test_verification.py compares the regenerated distances with the
fixture's stored ones and fails in that case.  Regenerate the fixture (python tools/make_golden.py verification) with any change."""
import numpy as np


def synthetic_pairs(n_pairs: int, dim: int, seed: int, layout: str = "blocks", flip: bool = True):
    """A synthetic verification set for tests, fixtures and benchmarks: (emb0, emb1 or None) fp32 [2P, D] and issame [P] bool.  Genuine
    pairs share a base vector under noise of a per-pair level in [0.3, 6], impostor pairs are independent; ``layout``: 'blocks'
    (runs of 300 genuine / 300 impostor pairs like lfw), 'alternate' or 'random' (30 % genuine)."""
    rng = np.random.default_rng(seed)
    p = np.arange(n_pairs)
    if layout == "blocks":
        issame = (p // 300) % 2 == 0
    elif layout == "alternate":
        issame = p % 2 == 0
    elif layout == "random":
        issame = rng.random(n_pairs) < 0.3
    else:
        raise ValueError(layout)
    base = rng.standard_normal((n_pairs, dim))
    level = rng.uniform(0.3, 6.0, (n_pairs, 1))
    first = base + 0.1 * rng.standard_normal((n_pairs, dim))
    second = np.where(issame[:, None], base + level * rng.standard_normal((n_pairs, dim)), rng.standard_normal((n_pairs, dim)))
    emb0 = np.empty((2 * n_pairs, dim), np.float32)
    emb0[0::2], emb0[1::2] = first, second
    emb0 *= rng.uniform(5.0, 30.0, (2 * n_pairs, 1)).astype(np.float32)
    emb1 = (emb0 + 0.05 * np.abs(emb0).mean() * rng.standard_normal(emb0.shape)).astype(np.float32) if flip else None
    return emb0, emb1, issame
