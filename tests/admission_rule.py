"""The admission rule of the scanning coded kinds (PQ<M>, SQ8, IVF<n>,PQ<M>, IVF<n>,SQ8), stated once for their CPU models.  A helper
module: nothing here is collected.

FAISS collects a query's results in a heap that starts full of (neutral, -1), neutral = FLT_MAX under L2 and -FLT_MAX under inner
product, and lets a value in only if it is STRICTLY better than the heap's worst: `top > dis` (L2), `top < dis` (inner product), both f32
comparisons.  Whatever the heap holds later is better than neutral, so a value the rule refuses against neutral is refused always:
a NaN (every comparison with it is false), +inf and FLT_MAX under L2, -inf and -FLT_MAX under inner product.  Their slots stay (neutral, -1).
Among the values the rule admits the coded kinds keep the k best in their pure order; the models sort for that."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
METRIC_INNER_PRODUCT, METRIC_L2 = 0, 1  # (oracle/oracle.py)


def admitted(metric, dis):
    """bool mask over dis (any shape, f32): the values FAISS's heap can ever hold"""
    dis = np.asarray(dis)
    assert dis.dtype == np.float32, dis.dtype
    with np.errstate(invalid="ignore"):
        return dis < FLT_MAX if metric == METRIC_L2 else dis > -FLT_MAX
