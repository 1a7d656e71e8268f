"""Host side of the polygon output: the ring table and the vertices of loops.polygons grouped into polygons and
written as GeoJSON (RFC 7946).  numpy and json only; nothing here touches the device.

  ring table   int64 [rings][7], rings by ascending id: (id, label, byte, first vertex, vertex count, crack count, A2); A2 the doubled
               signed area in pixel-corner coordinates, y down: > 0 an exterior ring, < 0 a hole
  vertices     int32 [n][2] = (X, Y), ring after ring in table order"""
import json

import numpy as np

ID, LABEL, BYTE, FIRST, VERTICES, CRACKS, A2 = range(7)
IDENTITY = (1, 0, 0, 0, 1, 0)


def polygons_of(ring_table, vertices):
    """The rings grouped by component: a list of (byte, label, exterior, [holes]) by ascending label, every ring an int32 array
    [n][2] of its vertices (not closed), the holes by ascending id.  Every label must have exactly one ring with A2 > 0 -- what
    drs_polygon_rings writes always has --, else ValueError."""
    table = np.asarray(ring_table, dtype=np.int64).reshape(-1, 7)
    vertices = np.asarray(vertices).reshape(-1, 2)
    groups = {}
    for row in table:
        ring = vertices[int(row[FIRST]):int(row[FIRST] + row[VERTICES])]
        if len(ring) != row[VERTICES]:
            raise ValueError("ring %d: its vertices %d..%d lie outside the %d given" % (row[ID], row[FIRST], row[FIRST] + row[VERTICES], len(vertices)))
        g = groups.setdefault(int(row[LABEL]), {"byte": int(row[BYTE]), "exterior": [], "holes": []})
        if g["byte"] != row[BYTE]:
            raise ValueError("component %d: rings of byte %d and of byte %d" % (row[LABEL], g["byte"], row[BYTE]))
        g["exterior" if row[A2] > 0 else "holes"].append(ring)
    out = []
    for label in sorted(groups):
        g = groups[label]
        if len(g["exterior"]) != 1:
            raise ValueError("component %d: %d rings of positive area, expected exactly 1" % (label, len(g["exterior"])))
        out.append((g["byte"], label, g["exterior"][0], g["holes"]))
    return out


def _sums(ring_table):
    """{label: (pixels = sum A2 / 2, perimeter = sum of crack counts)} over all rings of a component"""
    table = np.asarray(ring_table, dtype=np.int64).reshape(-1, 7)
    sums = {}
    for row in table:
        a, c = sums.get(int(row[LABEL]), (0, 0))
        sums[int(row[LABEL])] = (a + int(row[A2]), c + int(row[CRACKS]))
    return {k: (a // 2, c) for k, (a, c) in sums.items()}


def geojson(ring_table, vertices, K, class_names=None, transform=None):
    """A GeoJSON FeatureCollection (a dict): one Polygon feature per component whose byte is < K -- bytes >= K, such as an ignore
    label, are skipped --, by ascending label.  Rings are closed (the first point repeated), the exterior first.  Properties: class,
    class_name (if class_names is given), component (the label: the smallest pixel index y w + x), pixels (sum A2 / 2 over its rings)
    and perimeter (the crack count of all its rings, in pixel sides).  transform = (a, b, c, d, e, f) maps a corner (X, Y) to
    (a X + b Y + c, d X + e Y + f) in float64; the default is the identity and leaves the integers as they are: pixel corners, y down.
    When a e - b d < 0 every ring is written reversed, so that an exterior ring has positive shoelace area in the written coordinates
    whatever the transform (RFC 7946's orientation)."""
    identity = transform is None
    if not identity and len(transform) != 6:
        raise ValueError("transform %r: expected 6 numbers (a, b, c, d, e, f)" % (transform,))
    a, b, c, d, e, f = IDENTITY if identity else [float(v) for v in transform]
    flip = a * e - b * d < 0
    if class_names is not None and len(class_names) < K:
        raise ValueError("class_names: %d names for %d classes" % (len(class_names), K))
    sums = _sums(ring_table)

    def coords(ring):
        ring = np.asarray(ring)
        if identity:
            pts = [[int(x), int(y)] for x, y in ring]
        else:
            x, y = ring[:, 0].astype(np.float64), ring[:, 1].astype(np.float64)
            pts = [[float(u), float(v)] for u, v in zip(a * x + b * y + c, d * x + e * y + f)]
        pts.append(pts[0])
        if flip:
            pts.reverse()                  # the closed ring backwards: it still starts at the ring's first vertex
        return pts
    features = []
    for byte, label, exterior, holes in polygons_of(ring_table, vertices):
        if byte >= K:
            continue
        props = {"class": byte}
        if class_names is not None:
            props["class_name"] = str(class_names[byte])
        props.update(component=label, pixels=sums[label][0], perimeter=sums[label][1])
        features.append({"type": "Feature", "properties": props,
                         "geometry": {"type": "Polygon", "coordinates": [coords(exterior)] + [coords(r) for r in holes]}})
    return {"type": "FeatureCollection", "features": features}


def write_geojson(path, ring_table, vertices, K, class_names=None, transform=None):
    """geojson(...) written to `path` with json; returns the dict.  Under the identity transform every coordinate is written as an
    integer."""
    doc = geojson(ring_table, vertices, K, class_names=class_names, transform=transform)
    with open(path, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    return doc
