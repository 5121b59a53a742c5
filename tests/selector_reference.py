"""numpy model of the selector programs (include/mi355_faiss.h "selector programs"): the nested-tuple form that mi355_faiss.make_params
accepts, evaluated over an array of ids.

    ("all",) | ("range", a, b) | ("bitmap", uint8 array) | ("batch", ids) | ("array", ids)
    ("not", s) | ("and", s, t) | ("or", s, t) | ("xor", s, t)

mask(ids, tree) is the bool membership per id, admitted(ids, tree) the admitted ids in the order given (duplicates kept), postfix(tree) the
program's nodes as (op number, array or None, imin, imax) -- the MVS_SELOP_* numbers of the header -- and random_tree() a generator for the
tests."""

import numpy as np

OPS = {"all": 1, "bitmap": 2, "batch": 3, "array": 4, "range": 5, "not": 6, "and": 7, "or": 8, "xor": 9}


def mask(ids, tree):
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    kind = tree[0]
    if kind == "all":
        return np.ones(ids.shape, dtype=bool)
    if kind == "range":
        return (ids >= np.int64(tree[1])) & (ids < np.int64(tree[2]))
    if kind == "bitmap":  # the id read as uint64; beyond the bitmap is no member
        bits = np.ascontiguousarray(tree[1], dtype=np.uint8)
        u = ids.view(np.uint64)
        byte = u >> np.uint64(3)
        inside = byte < np.uint64(bits.size)
        out = np.zeros(ids.shape, dtype=bool)
        if bits.size:
            b = bits[np.where(inside, byte, 0).astype(np.int64)]
            out = inside & (((b >> (u & np.uint64(7)).astype(np.uint8)) & 1) == 1)
        return out
    if kind in ("batch", "array"):
        return np.isin(ids, np.ascontiguousarray(tree[1], dtype=np.int64))
    if kind == "not":
        return ~mask(ids, tree[1])
    a, b = mask(ids, tree[1]), mask(ids, tree[2])
    if kind == "and":
        return a & b
    if kind == "or":
        return a | b
    if kind == "xor":
        return a ^ b
    raise ValueError(kind)


def admitted(ids, tree):
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    return ids[mask(ids, tree)]


def postfix(tree, out=None):
    out = [] if out is None else out
    kind = tree[0]
    if kind in ("not", "and", "or", "xor"):
        for sub in tree[1:]:
            postfix(sub, out)
        out.append((OPS[kind], None, 0, 0))
    elif kind == "range":
        out.append((OPS[kind], None, int(tree[1]), int(tree[2])))
    elif kind == "all":
        out.append((OPS[kind], None, 0, 0))
    elif kind == "bitmap":
        out.append((OPS[kind], np.ascontiguousarray(tree[1], dtype=np.uint8), 0, 0))
    else:
        out.append((OPS[kind], np.ascontiguousarray(tree[1], dtype=np.int64), 0, 0))
    return out


def bitmap_of(ids, nbytes=None):
    """the IDSelectorBitmap bytes with exactly the bits of `ids` (all >= 0) set"""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    n = (int(ids.max()) >> 3) + 1 if ids.size else 0
    bits = np.zeros(max(n, nbytes or 0), dtype=np.uint8)
    if ids.size:
        np.bitwise_or.at(bits, ids >> 3, (1 << (ids & 7)).astype(np.uint8))
    return bits


def random_tree(rng, pool, depth):
    """a random tree of at most `depth` levels whose leaves draw their ids, bounds and bits from `pool` (an int64 array)"""
    pool = np.ascontiguousarray(pool, dtype=np.int64)
    if depth <= 1 or rng.random() < 0.25:
        leaf = rng.integers(0, 5)
        if leaf == 0:
            return ("all",)
        if leaf == 1:
            a, b = np.sort(rng.choice(pool, 2))
            return ("range", int(a), int(b))
        if leaf == 2:
            small = pool[(pool >= 0) & (pool < 1 << 16)]
            pick = small[rng.random(small.size) < 0.5]
            return ("bitmap", bitmap_of(pick, int(rng.integers(0, 3))))
        pick = pool[rng.random(pool.size) < rng.choice([0.05, 0.5])]
        if pick.size and rng.random() < 0.5:
            pick = np.concatenate([pick, pick[:3]])  # duplicates are harmless
        return ("batch" if leaf == 3 else "array", rng.permutation(pick))
    op = ("not", "and", "or", "xor")[rng.integers(0, 4)]
    if op == "not":
        return ("not", random_tree(rng, pool, depth - 1))
    return (op, random_tree(rng, pool, depth - 1), random_tree(rng, pool, depth - 1))
