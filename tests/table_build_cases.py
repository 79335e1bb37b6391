"""The pairs the table build's CPU and GPU tests are made of."""
import numpy as np

from dlsm_amd import index_block as ib

KEYS = {"k28": lambda j: 28, "k8": lambda j: 8, "var": lambda j: 8 if j == 0 else 15 + (j * 37) % 126}
VALUES = {"v0": lambda j: 0, "v1": lambda j: 1, "v15": lambda j: 15, "v16": lambda j: 16, "v17": lambda j: 17,
          "v400": lambda j: 400, "mix": lambda j: 0 if (j // 7) % 3 == 0 else (j * 131) % 601}


def make(n, klen, vlen, seed=3):
    """n pairs in key order: internal keys of klen(j) bytes, values of vlen(j)."""
    rng = np.random.default_rng(seed)
    blob = rng.integers(0, 256, 1 << 16, dtype=np.uint8).tobytes()
    iks = [ib.internal_key((b"%07d" % j + blob[j:j + 200])[:klen(j) - 8] if klen(j) > 8 else b"", 10 ** 6 - j, j % 5 != 2)
           for j in range(n)]
    return iks, [blob[3 * j:3 * j + vlen(j)] for j in range(n)]
