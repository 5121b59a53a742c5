"""The Python model of remove_ids (include/mi355_faiss.h "remove_ids") -- test infrastructure only.

It restates, in the plainest code that will do, what the library promises:
  stable compaction        Flat, PQ<M>, SQ8 (row r goes iff label_offset + r is a member) and IDMap over them (iff id_map[r] is);
  the swap loop            every inverted list of an IVF kind, written literally as FAISS's
                               l = size; j = 0; while (j < l) { if member(ids[j]) { --l; ids[j] = ids[l]; codes[j] = codes[l]; } else ++j; }
  the renumbering          IDMap over an IVF kind: stored id s goes iff id_map[s] is a member, survivors become s - #{removed r < s}.

remove_image works on the image dictionaries of tests/faiss_format.py (loads / dumps) -- flat, idmap, ivfflat and idmap over them -- and
returns the new image; survivors(image) gives the rows (and stored ids) in the resulting order, which is the order a fresh index has to be
filled in to behave the same.  The code kinds (PQ, SQ8 and their IVF forms), which faiss_format does not parse, use the same pieces on arrays:
stable_keep for the stores, remove_lists for the inverted lists."""
import copy

import numpy as np


def members(sel, ids):
    """boolean mask: which of `ids` are members of sel = ("bitmap", uint8 array) | ("batch", int64 array)"""
    kind, data = sel
    ids = np.asarray(ids, dtype=np.int64)
    if kind == "bitmap":
        bits = np.ascontiguousarray(data, dtype=np.uint8)
        out = np.zeros(ids.shape, dtype=bool)
        for i, v in enumerate(ids.tolist()):
            if v >= 0 and (v >> 3) < bits.size:  # a negative id or one beyond the bitmap is no member
                out[i] = (int(bits[v >> 3]) >> (v & 7)) & 1
        return out
    if kind == "batch":
        return np.isin(ids, np.asarray(data, dtype=np.int64))
    raise ValueError(kind)


def stable_keep(ids, sel):
    """positions of the survivors, in order: the rows whose id is no member"""
    return np.nonzero(~members(sel, ids))[0]


def swap_loop(ids, is_member):
    """FAISS's loop over one list, literally.  Returns the ORIGINAL positions of the survivors in their new order."""
    ids = [int(v) for v in ids]
    pos = list(range(len(ids)))
    l, j = len(ids), 0
    while j < l:
        if is_member(ids[j]):
            l -= 1
            ids[j] = ids[l]
            pos[j] = pos[l]
        else:
            j += 1
    return pos[:l]


def remove_lists(list_ids, sel, id_map=None):
    """list_ids: one int64 array of stored ids per list.  Returns (orders, new_ids, removed, keep_by_id):
    orders[l] = original positions of list l's survivors in their new order, new_ids[l] their stored ids (renumbered under id_map),
    keep_by_id = the survivors by stored id under id_map (else None)"""
    if id_map is None:
        gone = {int(v) for l in list_ids for v, m in zip(np.asarray(l).tolist(), members(sel, l).tolist()) if m}
        renum, keep_by_id = None, None
    else:
        id_map = np.asarray(id_map, dtype=np.int64)
        stored = np.sort(np.concatenate([np.asarray(l, dtype=np.int64) for l in list_ids]) if len(list_ids) else np.zeros(0, np.int64))
        if not np.array_equal(stored, np.arange(id_map.size)):
            raise ValueError("stored ids are not exactly 0 .. ntotal-1, each once")
        m = members(sel, id_map)
        gone = set(np.nonzero(m)[0].tolist())
        keep_by_id = ~m
        renum = np.cumsum(keep_by_id) - keep_by_id  # s - #{removed r < s}
    orders, new_ids, removed = [], [], 0
    for l in list_ids:
        l = np.asarray(l, dtype=np.int64)
        order = swap_loop(l, lambda v: v in gone)
        removed += l.size - len(order)
        ids = l[order] if len(order) else np.zeros(0, np.int64)
        orders.append(np.asarray(order, dtype=np.int64))
        new_ids.append(renum[ids].astype(np.int64) if renum is not None else ids)
    return orders, new_ids, removed, keep_by_id


def _remove_ivf(img, sel, id_map):
    orders, new_ids, removed, keep_by_id = remove_lists([ids for ids, _ in img["lists"]], sel, id_map)
    out = copy.deepcopy(img)
    out["lists"] = [(new_ids[l], np.ascontiguousarray(codes[orders[l]]).reshape(-1, img["d"])) for l, (_, codes) in enumerate(img["lists"])]
    out["ntotal"] = img["ntotal"] - removed
    return out, removed, keep_by_id


def remove_image(img, sel, label_offset=0):
    """image dictionary (faiss_format.loads) -> (the image after remove_ids(sel), rows removed)"""
    k = img["kind"]
    if k == "flat":
        keep = stable_keep(label_offset + np.arange(img["ntotal"]), sel)
        out = copy.deepcopy(img)
        out["x"] = np.ascontiguousarray(img["x"][keep])
        out["ntotal"] = int(keep.size)
        return out, img["ntotal"] - int(keep.size)
    if k == "ivfflat":
        out, removed, _ = _remove_ivf(img, sel, None)
        return out, removed
    if k == "idmap":
        sub = img["sub"]
        out = copy.deepcopy(img)
        if sub["kind"] == "flat":
            keep = stable_keep(img["ids"], sel)
            out["sub"]["x"] = np.ascontiguousarray(sub["x"][keep])
            out["sub"]["ntotal"] = int(keep.size)
            out["ids"] = np.asarray(img["ids"], dtype=np.int64)[keep]
            removed = img["ntotal"] - int(keep.size)
        elif sub["kind"] == "ivfflat":
            out["sub"], removed, keep_by_id = _remove_ivf(sub, sel, img["ids"])
            out["ids"] = np.asarray(img["ids"], dtype=np.int64)[keep_by_id]
        else:
            raise ValueError("remove_ids not implemented for this type of index")
        out["ntotal"] = img["ntotal"] - removed
        return out, removed
    raise ValueError("remove_ids not implemented for this type of index")


def survivors(img):
    """(rows [n, d], stored ids or None, external ids or None) in the order a fresh index is filled in: Flat rows as they are, IVF rows
    list by list (the state ivf_from_host produces)"""
    k = img["kind"]
    if k == "flat":
        return img["x"], None, None
    if k == "ivfflat":
        rows = [c for _, c in img["lists"] if len(c)]
        ids = [i for i, _ in img["lists"] if len(i)]
        d = img["d"]
        return (np.concatenate(rows) if rows else np.zeros((0, d), np.float32)), (np.concatenate(ids) if ids else np.zeros(0, np.int64)), None
    if k == "idmap":
        rows, stored, _ = survivors(img["sub"])
        ext = np.asarray(img["ids"], dtype=np.int64)
        return rows, stored, (ext if stored is None else ext[stored])
    raise ValueError(k)


def same_image(a, b):
    """field-by-field equality of two image dictionaries; floats as bit patterns"""
    if a["kind"] != b["kind"] or a["ntotal"] != b["ntotal"] or a["d"] != b["d"] or a["metric"] != b["metric"]:
        return False
    k = a["kind"]
    if k == "flat":
        return np.array_equal(a["x"].view(np.uint32), b["x"].view(np.uint32))
    if k == "idmap":
        return np.array_equal(a["ids"], b["ids"]) and same_image(a["sub"], b["sub"])
    if k == "ivfflat":
        if a["nlist"] != b["nlist"] or a["nprobe"] != b["nprobe"] or a["is_trained"] != b["is_trained"] or len(a["lists"]) != len(b["lists"]):
            return False
        if not same_image(a["quantizer"], b["quantizer"]):
            return False
        return all(np.array_equal(ia, ib) and np.array_equal(np.ascontiguousarray(ca, np.float32).view(np.uint32).reshape(-1), np.ascontiguousarray(cb, np.float32).view(np.uint32).reshape(-1))
                   for (ia, ca), (ib, cb) in zip(a["lists"], b["lists"]))
    if k == "hnswflat":
        ga, gb = a["graph"], b["graph"]
        return all(np.array_equal(np.asarray(ga[f]), np.asarray(gb[f])) for f in ga) and same_image(a["storage"], b["storage"])
    raise ValueError(k)
