"""Exact stand-in of gr_member_outlines, written independently of the device code: Python integers,
one dictionary of directed-edge counts per class built from the (face, class) members, then the cancellation, the successor and a
plain ring walk of X4-X6 class by class.  `StandInBackend` adds `member_outlines` to the stand-in backend of outline_standin.py,
for host-logic tests; the membership builders at the end are shared by the host and the device tests.
"""
import numpy as np

from outline_standin import STAT_WORDS, _area2
from outline_standin import StandInBackend as _ClassBackend

BAD_ROWS = 6                     # the statistics word of Y2
MEMBER_MAX_CLASSES = 2 ** 31 - 2


def bad_ptr(face_ptr, nnz, n_faces):
    """Y2, the offsets alone: face_ptr[0] != 0, face_ptr[F] != nnz, and every face whose row ends before it starts."""
    ptr = [int(p) for p in np.asarray(face_ptr).reshape(-1)]
    assert len(ptr) == n_faces + 1
    return (ptr[0] != 0) + (ptr[n_faces] != nnz) + sum(ptr[f + 1] < ptr[f] for f in range(n_faces))


def bad_rows(face_ptr, face_members, n_faces):
    """Y2: the number of violations of a well-formed table -- those of the offsets and, in every row (clamped into the table),
    the members that do not exceed the one before.  With malformed offsets the rows overlap or leave gaps and the device counts
    the order of the members against the rows as its waves meet them: then only `bad_ptr` of the count is defined."""
    ptr = [int(p) for p in np.asarray(face_ptr).reshape(-1)]
    members = [int(c) for c in np.asarray(face_members).reshape(-1)]
    nnz = len(members)
    bad = bad_ptr(ptr, nnz, n_faces)
    for f in range(n_faces):
        lo = min(max(ptr[f], 0), nnz)
        hi = min(max(ptr[f + 1], lo), nnz)
        bad += sum(members[m - 1] >= members[m] for m in range(lo + 1, hi))
    return bad


def members_np(verts_q, faces, face_ptr, face_members, n_classes):
    """{"canon", "ring_vertices", "ring_offsets", "ring_class", "stats", "n_edges", "n_rings"}: Y1-Y5.  A malformed table gives
    the count of its violations and nothing else, as the device does."""
    xy = [(int(x), int(y)) for x, y in np.asarray(verts_q, dtype=np.int64).reshape(-1, 2)]
    tris = np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist()
    ptr = [int(p) for p in np.asarray(face_ptr).reshape(-1)]
    members = [int(c) for c in np.asarray(face_members).reshape(-1)]
    V = len(xy)
    first, canon = {}, []
    for i, p in enumerate(xy):   # X2
        canon.append(first.setdefault(p, i))
    stats = [0] * STAT_WORDS
    stats[5] = sum(any(v < 0 or v >= V for v in tri) for tri in tris)   # BAD_FACES counts faces, with or without members
    stats[BAD_ROWS] = bad_rows(ptr, members, len(tris))
    per_class = {}   # class -> {(a, b): copies}
    if not stats[BAD_ROWS]:
        for f, tri in enumerate(tris):   # Y3
            if any(v < 0 or v >= V for v in tri):
                continue
            a, b, d = (canon[v] for v in tri)
            area = _area2(xy[a], xy[b], xy[d])
            if area < 0:
                b, d = d, b
            for c in members[ptr[f]:ptr[f + 1]]:
                if not 0 <= c < n_classes:
                    stats[0] += 1
                elif area == 0:
                    stats[1] += 1
                else:
                    stats[2] += area < 0
                    count = per_class.setdefault(c, {})
                    for e in ((a, b), (b, d), (d, a)):
                        count[e] = count.get(e, 0) + 1
    ring_vertices, offsets, ring_class = [], [0], []
    for c in sorted(per_class):   # Y4: X4-X6 within the class; Y5: class after class
        count = per_class[c]
        slots = []
        for (a, b), n in count.items():   # X4
            back = count.get((b, a), 0)
            if a < b:
                stats[3] += min(n, back)
            stats[4] += n - back > 1
            slots += [(a, b, copy) for copy in range(n - back)]
        slots.sort()
        coming, going = {}, {}
        for s, (a, b, copy) in enumerate(slots):   # X5
            coming.setdefault(b, []).append((a, copy, s))
            going.setdefault(a, []).append((b, copy, s))
        follower = [None] * len(slots)
        for vertex, inc in coming.items():
            out = going.get(vertex, [])
            assert len(inc) == len(out), "X5: a (class, vertex) with unequal incoming and outgoing copies"
            for (_, _, s), (_, _, t) in zip(sorted(inc), sorted(out)):
                follower[s] = t
        seen = [False] * len(slots)
        for s in range(len(slots)):   # X6: leaders ascend, so the rings of the class come out in their order
            if seen[s]:
                continue
            t = s
            while not seen[t]:
                seen[t] = True
                ring_vertices.append(slots[t][0])
                t = follower[t]
            assert t == s, "X5 is a bijection: the walk comes back to its start"
            offsets.append(len(ring_vertices))
            ring_class.append(c)
    return {
        "canon": np.array(canon, dtype=np.int32).reshape(-1),
        "ring_vertices": np.array(ring_vertices, dtype=np.int32).reshape(-1),
        "ring_offsets": np.array(offsets, dtype=np.int64),
        "ring_class": np.array(ring_class, dtype=np.int32).reshape(-1),
        "stats": np.array(stats, dtype=np.int64),
        "n_edges": len(ring_vertices), "n_rings": len(ring_class),
    }


class StandInBackend(_ClassBackend):
    """`HipRaster.class_outlines` and `HipRaster.member_outlines` on the CPU; counts the calls of each."""

    def member_outlines(self, verts_q, faces, face_ptr, face_members, n_classes, capacity=None, check=True):
        host = lambda a: np.asarray(a.cpu() if hasattr(a, "detach") else a)
        verts_q, faces, face_ptr, face_members = host(verts_q), host(faces), host(face_ptr), host(face_members)
        if not 0 <= int(n_classes) <= MEMBER_MAX_CLASSES:
            raise ValueError(f"gr_member_outlines: n_classes={int(n_classes)} outside [0, {MEMBER_MAX_CLASSES}]")
        if 3 * len(face_members) >= 2 ** 31:
            raise ValueError(f"gr_member_outlines: {len(face_members)} members, one call takes fewer than 2^31 / 3")
        self.last_members = dict(verts_q=verts_q, faces=faces, face_ptr=face_ptr, face_members=face_members, n_classes=int(n_classes))
        self.member_calls = getattr(self, "member_calls", 0) + 1
        got = members_np(verts_q, faces, face_ptr, face_members, int(n_classes))
        if check and got["stats"][5]:
            raise ValueError(f"gr_member_outlines: {int(got['stats'][5])} faces name a vertex outside [0, {len(verts_q)})")
        if check and got["stats"][BAD_ROWS]:
            raise ValueError(f"gr_member_outlines: {int(got['stats'][BAD_ROWS])} violations of a well-formed member table")
        return got["canon"], got["ring_vertices"], got["ring_offsets"], got["ring_class"], got["stats"]


# -- memberships shared by the host and the device tests --------------------------------------------------------------------------------
def csr_of_rows(rows):
    """rows: for every face the list of its classes -> (face_ptr (F + 1,) int64, face_members (nnz,) int32), rows sorted."""
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(set(r)) for r in rows])
    flat = [c for r in rows for c in sorted(set(r))]
    return ptr, np.array(flat, dtype=np.int32).reshape(-1)


def column_classes(face_ptr, face_members, column, n_faces):
    """face_class of Y5's "alone": 0 where the face is a member of `column`, -1 elsewhere."""
    out = np.full(n_faces, -1, dtype=np.int32)
    rows = np.repeat(np.arange(n_faces), np.diff(face_ptr))
    out[rows[np.asarray(face_members) == column]] = 0
    return out


def random_rows(n_faces, n_classes, seed, most=3):
    """0 .. most classes per face, drawn without repetition."""
    rng = np.random.default_rng(seed)
    return [sorted(rng.choice(n_classes, size=int(rng.integers(0, most + 1)), replace=False).tolist()) for _ in range(n_faces)]


def rows_with_nnz(n_faces, n_classes, nnz, seed):
    """Random rows that hold exactly nnz members in all (nnz <= n_faces n_classes)."""
    rng = np.random.default_rng(seed)
    cells = rng.choice(n_faces * n_classes, size=nnz, replace=False)
    rows = [[] for _ in range(n_faces)]
    for cell in sorted(cells.tolist()):
        rows[cell // n_classes].append(cell % n_classes)
    return rows
