"""Rule 10 of include/pt_hip.h -- the refit of a BVH from new primitive boxes -- in numpy, written twice: refit()
works on whole arrays, one depth at a time as the device does; refit_by_node() walks the tree node by node with
scalars.  Both use compares and selects only, in the rule's own order, so they agree word for word and with the
device (no tolerance anywhere).

A tree is four arrays: lo, hi (n x 3 float32), offset, pca (n uint32; pca = primitive_count_axis of pt_bvh_node: the
primitive count in the high 16 bits, a leaf when it is not 0).  An interior node's children are i + 1 and offset[i].
Boxes are (prim_count x 6) float32: min xyz, max xyz.  tests/bvh_edit.py's node tuples convert with from_tuples() and
to_tuples().

records() restates the child-box records pt_set_scene makes (16 words per interior node in array order, zero for an
unreachable one) and refit_records() what the refit rewrites of them: quads 0-2 of reachable interior nodes.
"""
import numpy as np

F, U = np.float32, np.uint32


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(U)


def same_words(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def from_tuples(nodes):
    lo = np.array([n[0] for n in nodes], dtype=F).reshape(-1, 3)
    hi = np.array([n[1] for n in nodes], dtype=F).reshape(-1, 3)
    return lo, hi, np.array([n[2] for n in nodes], dtype=U), np.array([n[3] for n in nodes], dtype=U)


def to_tuples(lo, hi, offset, pca):
    return [(tuple(float(x) for x in lo[i]), tuple(float(x) for x in hi[i]), int(offset[i]), int(pca[i])) for i in range(len(offset))]


def depths(offset, pca):
    """Depth of every node reachable from the root (the root's is 0), -1 for an unreachable one."""
    d = np.full(len(offset), -1, dtype=np.int64)
    st = [(0, 0)]
    while st:
        i, k = st.pop()
        d[i] = max(d[i], k)
        if (int(pca[i]) >> 16) == 0:
            st.append((i + 1, k + 1))
            st.append((int(offset[i]), k + 1))
    return d


def refit(lo, hi, offset, pca, boxes):
    """Whole arrays: the leaves, then every depth of interior nodes from the deepest up.  Returns (lo, hi)."""
    lo, hi = np.array(lo, dtype=F), np.array(hi, dtype=F)
    boxes = np.asarray(boxes, dtype=F).reshape(-1, 6)
    offset, pca = np.asarray(offset, dtype=U), np.asarray(pca, dtype=U)
    d = depths(offset, pca)
    count = (pca >> 16).astype(np.int64)
    leaves = np.flatnonzero((d >= 0) & (count > 0))
    f = offset[leaves].astype(np.int64)
    l, h = boxes[f, :3].copy(), boxes[f, 3:].copy()
    for k in range(1, int(count[leaves].max())):
        on = count[leaves] > k
        b = boxes[np.where(on, f + k, f)]
        l = np.where(on[:, None] & (b[:, :3] < l), b[:, :3], l)
        h = np.where(on[:, None] & (b[:, 3:] > h), b[:, 3:], h)
    lo[leaves], hi[leaves] = l, h
    interior = (d >= 0) & (count == 0)
    for k in range(int(d.max()), -1, -1):
        i = np.flatnonzero(interior & (d == k))
        if len(i) == 0:
            continue
        a, b = i + 1, offset[i].astype(np.int64)
        lo[i] = np.where(lo[b] < lo[a], lo[b], lo[a])
        hi[i] = np.where(hi[b] > hi[a], hi[b], hi[a])
    return lo, hi


def refit_by_node(lo, hi, offset, pca, boxes):
    """Node by node from the root, children before their parent, scalars only.  Returns (lo, hi)."""
    lo, hi = np.array(lo, dtype=F), np.array(hi, dtype=F)
    boxes = np.asarray(boxes, dtype=F).reshape(-1, 6)
    post, st = [], [0]
    while st:
        i = st.pop()
        post.append(i)
        if (int(pca[i]) >> 16) == 0:
            st.append(i + 1)
            st.append(int(offset[i]))
    for i in reversed(post):             # reversed preorder: every child comes before its parent
        c = int(pca[i]) >> 16
        for ax in range(3):
            if c:
                f = int(offset[i])
                l, h = boxes[f, ax], boxes[f, 3 + ax]
                for k in range(1, c):
                    bl, bh = boxes[f + k, ax], boxes[f + k, 3 + ax]
                    l = bl if bl < l else l
                    h = bh if bh > h else h
            else:
                a, b = i + 1, int(offset[i])
                l = lo[b, ax] if lo[b, ax] < lo[a, ax] else lo[a, ax]
                h = hi[b, ax] if hi[b, ax] > hi[a, ax] else hi[a, ax]
            lo[i, ax], hi[i, ax] = l, h
    return lo, hi


def record_index(pca):
    """Record number of every node: interior nodes count up in array order, reachable or not; -1 for a leaf."""
    interior = (np.asarray(pca, dtype=U) >> 16) == 0
    return np.where(interior, np.cumsum(interior) - 1, -1)


def has_records(offset, pca, prim_count):
    """pt_set_scene keeps child-box records unless a reachable leaf holds more than 255 primitives (or the counts
    reach 2^24)."""
    d = depths(offset, pca)
    return bool(len(offset) < (1 << 24) and prim_count < (1 << 24) and not ((d >= 0) & ((np.asarray(pca) >> 16) > 255)).any())


def _first_prims(offset, pca, d):
    first = np.zeros(len(offset), dtype=np.int64)
    for i in range(len(offset) - 1, -1, -1):
        if d[i] < 0:
            continue
        first[i] = int(offset[i]) if (int(pca[i]) >> 16) else min(first[i + 1], first[int(offset[i])])
    return first


def records(lo, hi, offset, pca):
    """The records pt_set_scene makes: (max(interior, 1) x 16) float32."""
    d = depths(offset, pca)
    rec = record_index(pca)
    first = _first_prims(offset, pca, d)
    out = np.zeros((max(int((rec >= 0).sum()), 1), 16), dtype=F)
    w = out.view(U)

    def word(i):
        c = int(pca[i]) >> 16
        return ((c << 24) | int(offset[i])) if c else int(rec[i])

    for i in np.flatnonzero((rec >= 0) & (d >= 0)):
        a, b = i + 1, int(offset[i])
        w[rec[i], 12:] = [word(a), word(b), 1 << ((int(pca[i]) >> 8) & 0xFF), first[b]]
    return refit_records(out, lo, hi, offset, pca)


def refit_records(before, lo, hi, offset, pca):
    """Quads 0-2 of every reachable interior node's record from its children's boxes; everything else as before."""
    out = np.array(before, dtype=F)
    d = depths(offset, pca)
    rec = record_index(pca)
    for i in np.flatnonzero((rec >= 0) & (d >= 0)):
        a, b = i + 1, int(offset[i])
        out[rec[i], :12] = [lo[a, 0], hi[a, 0], lo[a, 1], hi[a, 1], lo[a, 2], hi[a, 2], lo[b, 2], hi[b, 2],
                            lo[b, 0], hi[b, 0], lo[b, 1], hi[b, 1]]
    return out
