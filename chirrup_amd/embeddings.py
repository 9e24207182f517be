"""Host half of a text embedding (DESIGN.md "Embeddings"): the worker's device kernel leaves, per request, the binary32 running sum
of the pooled binary16 ln_out rows, the last row and the row count; ``finish`` turns them into the vector a client gets.  Pure numpy
-- the worker and the tests share it."""
import numpy as np

POOLINGS = ("mean", "last")


def finish(sum_, last, count: int, pooling: str = "mean", normalize: bool = True) -> np.ndarray:
    """sum_: float32 [C] (sum of the pooled rows, accumulated in token order), last: float16 [C] (the last pooled row), count: rows
    pooled (>= 1).  mean: sum / count; last: the last row.  normalize: divided by its L2 norm (a zero vector stays zero).  The
    division and the normalisation run in binary64; the result is rounded ONCE, to binary32."""
    if pooling not in POOLINGS:
        raise ValueError(f"unknown pooling {pooling!r}, expected one of {', '.join(POOLINGS)}")
    count = int(count)
    if count < 1:
        raise ValueError("an embedding needs at least one pooled row")
    if pooling == "mean":
        e = np.asarray(sum_, dtype=np.float32).astype(np.float64) / np.float64(count)
    else:
        e = np.asarray(last, dtype=np.float16).astype(np.float64)
    if normalize:
        norm = np.sqrt(np.sum(e * e, dtype=np.float64))
        if norm > 0.0:
            e = e / norm
    return e.astype(np.float32)
