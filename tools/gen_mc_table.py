"""Generate csrc/mc_table.hpp, the marching-cubes case table of csrc/mc_extract.hpp:
    python tools/gen_mc_table.py            # rewrite the committed header
    python tools/gen_mc_table.py --check    # exit 1 when the committed header differs from what this writes
Nothing here is typed in from a published table; every row follows from the rule below (tests/test_mc_cpu.py regenerates the
header and checks the rule's consequences for all 256 cases).

Numbering.  Corner b of a cell sits at offset (di, dj, dk) = (b & 1, (b >> 1) & 1, (b >> 2) & 1) from the cell's grid
point.  Bit b of the case index is set when corner b is BELOW (v < iso).  Cube edge e = 4 * axis + idx runs along `axis`
from its owner corner, whose two other offsets, in increasing axis order, are (idx & 1, idx >> 1): the owner is the grid
point that owns the edge's vertex.

Rule, per case:
  1. on each of the six faces join the crossing edges (ends on different sides) into segments: two crossings give one
     segment; four (the face's below corners are diagonal) give two, each joining the two face edges at one BELOW corner,
     i.e. cutting that corner off.  Only the face's four flags are read, so the two cells sharing a face agree;
  2. every crossing edge lies on two faces and so ends two segments: chain them into closed loops;
  3. walk each loop so that its right-hand normal points from the above side to the below side.  On a face with outward
     normal f the surface's normal within the face is f x (direction of travel); it must point at the below end of the
     segment's first edge;
  4. loops in the order of their lowest edge number;
  5. a fan (A, Li, Li+1) from one edge A of the loop: the lowest-numbered one whose fan has no chord lying in a face of the
     cube.  Two crossing edges of one face that the face's segments do not join (the face is a diagonal one, and the loop
     passes it twice) would give such a chord; the neighbouring cell may draw the same chord, and the edge would then carry
     four triangles.  With no chord in a face, every triangle edge is either a face segment, drawn once by each of the two
     cells of the face, or strictly inside one cell: the surface is a closed manifold wherever it does not leave the volume.
     Every loop has such an edge (asserted below); for 18 of the 358 loops it is not the loop's lowest.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "imagesequenceregistrationfor6dposeestimationlabeling_amd", "csrc", "mc_table.hpp")

CORNERS = [(b & 1, (b >> 1) & 1, (b >> 2) & 1) for b in range(8)]


def corner_id(d):
    return d[0] | d[1] << 1 | d[2] << 2


def _edges():
    out = []
    for axis in range(3):
        o1, o2 = [a for a in range(3) if a != axis]
        for idx in range(4):
            d = [0, 0, 0]
            d[o1], d[o2] = idx & 1, idx >> 1
            c0 = corner_id(d)
            d[axis] = 1
            out.append((c0, corner_id(d)))
    return out


EDGES = _edges()                      # (owner corner, far corner)
FACES = [(axis, side) for axis in range(3) for side in range(2)]


def face_corners(face):
    axis, side = face
    return [b for b in range(8) if CORNERS[b][axis] == side]


def face_edges(face):
    on = set(face_corners(face))
    return [e for e, (a, b) in enumerate(EDGES) if a in on and b in on]


def below(case, corner):
    return bool(case >> corner & 1)


def crossing_edges(case):
    return [e for e, (a, b) in enumerate(EDGES) if below(case, a) != below(case, b)]


def face_segments(case, face):
    """The segments of one face: (edge, edge) pairs.  Reads the flags of the face's four corners only."""
    cross = [e for e in face_edges(face) if below(case, EDGES[e][0]) != below(case, EDGES[e][1])]
    if len(cross) == 2:
        return [tuple(cross)]
    if len(cross) == 4:
        return [tuple(e for e in cross if c in EDGES[e]) for c in face_corners(face) if below(case, c)]
    assert not cross
    return []


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def midpoint2(e):
    """Twice the midpoint of edge e (integers)."""
    a, b = CORNERS[EDGES[e][0]], CORNERS[EDGES[e][1]]
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def travel_sign(case, face, ea, eb):
    """> 0 when walking ea -> eb on `face` puts the below side on the side of f x travel (rule 3)."""
    axis, side = face
    f = [0, 0, 0]
    f[axis] = 2 * side - 1
    a, b = EDGES[ea]
    w = CORNERS[a if below(case, a) else b]
    A = midpoint2(ea)
    return _dot(_cross(tuple(f), _sub(midpoint2(eb), A)), _sub((2 * w[0], 2 * w[1], 2 * w[2]), A))


def loops(case):
    """The oriented loops of a case, each a list of cube edges starting at its lowest, in the order of those lowest edges."""
    at = {}                                       # edge -> its two (face, other edge)
    for face in FACES:
        for ea, eb in face_segments(case, face):
            at.setdefault(ea, []).append((face, eb))
            at.setdefault(eb, []).append((face, ea))
    assert sorted(at) == crossing_edges(case) and all(len(v) == 2 for v in at.values()), case
    out, seen = [], set()
    for start in sorted(at):
        if start in seen:
            continue
        face, nxt = next((f, o) for f, o in at[start] if travel_sign(case, f, start, o) > 0)
        loop, cur = [start], start
        while True:
            assert travel_sign(case, face, cur, nxt) > 0, (case, loop)
            if nxt == start:
                break
            loop.append(nxt)
            cur = nxt
            face, nxt = next((f, o) for f, o in at[cur] if f != face)
        assert len(loop) >= 3 and len(set(loop)) == len(loop), (case, loop)
        seen.update(loop)
        out.append(loop)
    return out


def share_a_face(ea, eb):
    return any(ea in face_edges(f) and eb in face_edges(f) for f in FACES)


def fan(loop):
    """Rule 5: the loop rotated to its apex, as triangles."""
    for apex in sorted(loop):
        r = loop[loop.index(apex):] + loop[:loop.index(apex)]
        if not any(share_a_face(r[0], r[i]) for i in range(2, len(r) - 1)):
            return [(r[0], r[i], r[i + 1]) for i in range(1, len(r) - 1)]
    raise AssertionError(("no fan without a chord in a face", loop))


def triangles(case):
    return [t for lp in loops(case) for t in fan(lp)]


def table():
    rows = [triangles(c) for c in range(256)]
    return rows, max(len(r) for r in rows)


def render():
    rows, width = table()
    lines = [
        "// mc_table.hpp — the marching-cubes case table.  GENERATED by tools/gen_mc_table.py (which states the rule): do not edit.",
        "// Corner b of a cell: offset (b & 1, (b >> 1) & 1, (b >> 2) & 1); bit b of the case: corner b is below (v < iso).",
        "// Cube edge e = 4 * axis + idx: along `axis` from its owner corner, whose other two offsets are (idx & 1, idx >> 1).",
        "// ISR_MC_TRI_EDGES: per case kMcMaxTris triangles of three cube edges, -1 past the case's count.",
        "#pragma once",
        "",
        f"#define ISR_MC_MAX_TRIS {width}",
        "",
        "#define ISR_MC_TRI_COUNTS \\",
    ]
    for r0 in range(0, 256, 32):
        lines.append("  " + ", ".join(str(len(rows[c])) for c in range(r0, r0 + 32)) + (", \\" if r0 + 32 < 256 else ""))
    lines += ["", "#define ISR_MC_TRI_EDGES \\"]
    for c, r in enumerate(rows):
        flat = [e for t in r for e in t] + [-1] * (3 * (width - len(r)))
        lines.append("  {" + ", ".join(f"{e:2d}" for e in flat) + "}" + (", \\" if c < 255 else ""))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    text = render()
    rows, width = table()
    print(f"largest triangle count of a case: {width}; triangles over all cases: {sum(len(r) for r in rows)}")
    if a.check:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("committed header is up to date" if same else "committed header DIFFERS")
        sys.exit(0 if same else 1)
    with open(HEADER, "w") as fh:
        fh.write(text)
    print(HEADER)


if __name__ == "__main__":
    main()
