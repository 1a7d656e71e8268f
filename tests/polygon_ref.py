"""The polygon outlines of a label map of DESIGN.md 8a.12 / include/drs.h (drs_polygon_count, drs_polygon_rings, drs_polygon_write;
loops.polygons) stated in numpy: sequential tracing.  Integer arithmetic throughout; numpy only.

  crack        side d of pixel p = y w + x whose pixel across is outside the map or carries another byte; id 4 p + d.  d = 0 top going
               east, 1 right going south, 2 bottom going west, 3 left going north: the pixel is on the right-hand side of travel
  succ         q = the pixel ahead of p in direction d, r = the pixel across side d of q, same = inside the map with p's byte;
               4: !same(q) -> (p, d + 1); !same(r) -> (q, d); else (r, d - 1).   8: same(r) -> (r, d - 1); same(q) -> (q, d); else (p, d + 1)
  ring         a cycle of succ, named by its smallest crack id; its vertices are the heads of the cracks whose successor goes another
               way, from the first such crack at or after the smallest one; A2 = sum x0 y1 - x1 y0 over its cracks (> 0 exterior, < 0 hole)
  table        int64 [rings][7], by ascending id: (id, label[id >> 2], m[id >> 2], first vertex, vertices, cracks, A2)
  vertices     int32 [n][2] = (X, Y), ring after ring"""
import numpy as np

import sieve_ref

DX, DY = np.array([1, 0, -1, 0]), np.array([0, 1, 0, -1])      # travel along side d; the pixel across side d lies at d - 1
HX, HY = np.array([1, 1, 0, 0]), np.array([0, 1, 1, 0])        # the crack's head corner relative to (x, y); its tail is that of d - 1


def _padded(m):
    pad = np.full((m.shape[0] + 2, m.shape[1] + 2), -1, dtype=np.int64)
    pad[1:-1, 1:-1] = m
    return pad


def cracks(m):
    """the ids of the map's cracks, ascending (int64)"""
    m = np.asarray(m)
    h, w = m.shape
    pad = _padded(m)
    across = (pad[:-2, 1:-1], pad[1:-1, 2:], pad[2:, 1:-1], pad[1:-1, :-2])
    p = np.arange(h * w, dtype=np.int64).reshape(h, w)
    return np.sort(np.concatenate([(4 * p + d)[across[d] != m] for d in range(4)]))


def succ(m, e, connectivity):
    """the ids of the cracks after the cracks e (an id or an array of ids)"""
    assert connectivity in (4, 8)
    m = np.asarray(m)
    h, w = m.shape
    pad = _padded(m)
    e = np.asarray(e, dtype=np.int64)
    p, d = e >> 2, e & 3
    y, x = p // w, p % w
    l = (d + 3) & 3
    qy, qx = y + DY[d], x + DX[d]
    ry, rx = qy + DY[l], qx + DX[l]
    b = pad[y + 1, x + 1]
    sq, sr = pad[qy + 1, qx + 1] == b, pad[ry + 1, rx + 1] == b          # outside the map is -1: never the same
    left = sr if connectivity == 8 else sq & sr
    return np.where(left, 4 * (ry * w + rx) + l, np.where(sq, 4 * (qy * w + qx) + d, 4 * p + ((d + 1) & 3)))


def rings(m, connectivity, label=None):
    """(table int64 [rings][7], vertices int32 [n][2]); label: that of sieve_ref.components(m, connectivity) if the caller has it.
    The cracks are walked one after the other from the smallest id not yet seen; the sums are then taken per walk."""
    m = np.asarray(m)
    h, w = m.shape
    if label is None:
        label = sieve_ref.components(m, connectivity)[0]
    ids = cracks(m)
    table_next = np.full(4 * h * w, -1, dtype=np.int64)
    table_next[ids] = succ(m, ids, connectivity)
    nxt, seen, order, start = table_next.tolist(), bytearray(4 * h * w), [], []
    for e0 in ids.tolist():
        if seen[e0]:
            continue
        start.append(len(order))
        e = e0
        while not seen[e]:
            seen[e] = 1
            order.append(e)
            e = nxt[e]
        assert e == e0                                                   # a cycle: the walk comes back to where it began
    order, start = np.array(order, dtype=np.int64), np.array(start, dtype=np.int64)
    p, d = order >> 2, order & 3
    x1, y1 = p % w + HX[d], p // w + HY[d]
    x0, y0 = p % w + HX[d - 1], p // w + HY[d - 1]
    turn = (table_next[order] & 3) != d
    first = np.concatenate([[0], np.cumsum(turn)])[start]
    e0 = order[start]
    table = np.stack([e0, label.reshape(-1)[e0 >> 2].astype(np.int64), m.reshape(-1)[e0 >> 2].astype(np.int64), first,
                      np.add.reduceat(turn.astype(np.int64), start), np.diff(np.concatenate([start, [len(order)]])),
                      np.add.reduceat(x0 * y1 - x1 * y0, start)], axis=1)
    return table.astype(np.int64), np.stack([x1[turn], y1[turn]], axis=1).astype(np.int32)


def fill(h, w, ring_list):
    """even-odd raster of rings (each an [n][2] array of (X, Y) corners, closed or not): bool [h][w], a pixel is inside iff an odd
    number of vertical ring edges lie to its left on its row"""
    flips = np.zeros((h, w + 1), dtype=np.int64)
    for r in ring_list:
        r = np.asarray(r, dtype=np.int64).reshape(-1, 2)
        for (xa, ya), (xb, yb) in zip(r, np.roll(r, -1, axis=0)):
            if xa == xb and ya != yb:
                flips[min(ya, yb):max(ya, yb), xa] += 1
    return (np.cumsum(flips, axis=1)[:, :w] & 1).astype(bool)


def ring_vertices(table, vertices):
    """the vertex arrays of the table's rings, in table order"""
    return [vertices[int(r[3]):int(r[3] + r[4])] for r in table]
