"""The list row pass of k_narrow<false> (tu_narrow.hip), probed: one wavefront runs up to four (flat face, hull) pairs, one per DPP row of 16
lanes, each row on the support-vertex list of the cell its first support direction falls into (HullSub, two entries per lane, policy G16).
Every row that reports its pair settled must have written the record the fused step's narrow_pair<NoCache, G64> writes, bit for bit.

Shared by tests/test_list_rows_emu.py (a subset, emulated) and tests/test_list_rows_gpu.py (everything, on the MI355X).

Per hull and per chosen cell (lists of 1, 15, 16, 17, 31, 32 entries, and one of 33, which the pass must not serve) seven poses whose first
support direction is the cell's centre, in this order, so that a wavefront of four holds a plane row next to box rows and a separated, an exact
and an unsettled row together:
  0 plane rest      the hull resting on the plane, 2 mm deep
  1 box rest        resting on the top face of a 1 x 1 x 0.25 m box, the deepest vertex over the face centre: exact
  2 box separated   the same, lifted 1 mm clear of the face: the face plane separates
  3 box margin out  the deepest vertex 1e-5 m OUTSIDE the outline-minus-margin boundary (|pu| = hu - d0 + 1e-5): a candidate, not exact - the
                    first face does not settle the pair
  4 plane tilted    pose 0 tilted by 1e-3 rad
  5 box margin in   the deepest vertex 1e-5 m inside that boundary: exact
  6 box tilted      pose 1 tilted by 1e-3 rad
The tie shapes (cube, 5 x 5 x 5 surface grid: dyadic coordinates) also rest on their six faces with exact rotations, where four to
twenty-five vertices tie for the deepest and the smallest index must win on every path.  Finite inputs only."""
import numpy as np

from tests import devprims
from tests import test_support_queries as sq
from tests.devprims import list_rows

F64 = np.float64
LENGTHS = (1, 15, 16, 17, 31, 32)
KINDS = ("plane rest", "box rest", "box separated", "box margin out", "plane tilted", "box margin in", "box tilted")
BOX = np.array([0.5, 0.5, 0.125])
D0 = 2e-3
EZ = np.array([0, 0, 1.0])


def scene_hull(blobs, name):
    from so101_sim_amd.model import blob as blobfmt
    m = blobfmt.unpack(blobs["f32"])
    g = blobs["meta"]["geom_names"].index(name)
    a, n = int(m["geom_vertadr"][g]), int(m["geom_vertnum"][g])
    return m["mesh_vert"].reshape(-1, 3).astype(np.float32)[a:a + n]


def hulls(blobs):
    """the smallest bowl piece (54 vertices), a bowl piece of about 300 (308), a banana part (498), and the tie shapes"""
    tie = sq.tie_hulls()
    out = {"bowl:54": scene_hull(blobs, "container/coacd_part_020"), "bowl:308": scene_hull(blobs, "container/coacd_part_016"),
           "banana:498": scene_hull(blobs, "object/coacd_part_002"), "cube:8": tie["cube:8"], "grid5:98": tie["grid5:98"]}
    assert [len(v) for v in out.values()] == [54, 308, 498, 8, 98]
    return out


def cell_centre(cell):
    face, iu, iv = cell // 64, (cell // 8) % 8, cell % 8
    ax, sg = face // 2, (-1.0 if face % 2 else 1.0)
    d = sg * np.eye(3)[ax] + (-1 + (iu + 0.5) / 4) * np.eye(3)[(ax + 1) % 3] + (-1 + (iv + 0.5) / 4) * np.eye(3)[(ax + 2) % 3]
    return d / np.linalg.norm(d)


def poses(V, R2):
    """the seven poses (g1, g2, rb, kind) of the hull V turned by R2 (its first support direction: R2' (-z))"""
    V64 = V.astype(F64)
    ctr, rb2 = V64.mean(0), float(np.linalg.norm(V64, axis=1).max())
    rb1 = float(np.linalg.norm(BOX))
    tilt = sq.rot_axis([np.cos(0.7), np.sin(0.7), 0], 1e-3)
    out = []

    def hull_at(R, p):
        return sq.pack_geom(sq.G_MESH, [0, 0, 0], R, p, R @ ctr + p)

    def plane(R):
        p2 = np.array([0.03, -0.02, -D0 - (V64 @ R.T)[:, 2].min()])
        return sq.pack_geom(sq.G_PLANE, [0, 0, 0], np.eye(3), [0, 0, 0], [0, 0, 0]), hull_at(R, p2), [0.0, rb2]

    def box(R, d0, pu):
        W = V64 @ R.T
        a0 = W[int(np.argmin(W[:, 2]))]                # (the deepest vertex; the first of a tie = the smallest index)
        if pu is not None and (R @ ctr - a0)[0] < 0:   # (the hull's centre stays inward of the vertex, so that the top face is visited first)
            pu = -pu
        p2 = np.array([(0.0 if pu is None else pu) - a0[0], -a0[1], BOX[2] - d0 - a0[2]])
        return sq.pack_geom(sq.G_BOX, BOX, np.eye(3), [0, 0, 0], [0, 0, 0]), hull_at(R, p2), [rb1, rb2]

    edge = -(BOX[0] - D0)
    for kind, g in zip(KINDS, (plane(R2), box(R2, D0, None), box(R2, -1e-3, None), box(R2, D0, edge - 1e-5), plane(tilt @ R2),
                               box(R2, D0, edge + 1e-5), box(tilt @ R2, D0, None))):
        out.append((*g, kind))
    return out


def cases(probes, H, V, lengths, tie):
    """(g1, g2, rb, kind) arrays: the seven poses at the centre of one cell per list length in `lengths` that the hull has, and for a tie
    shape its six faces down (exact rotations)"""
    L = np.diff(H.off.astype(np.int64))
    rows = []
    for n in lengths:
        cells = np.flatnonzero(L == n)
        if len(cells):
            d = cell_centre(int(cells[len(cells) // 2]))
            rows += poses(V, sq.rot_axis(EZ, 0.4) @ sq.rot_to(d, -EZ))
    if tie:
        for d in np.concatenate([np.eye(3), -np.eye(3)]):
            rows += poses(V, sq.rot_to(d, -EZ))
    g1, g2, rb, kind = (np.array(x) for x in zip(*rows))
    return g1, g2, rb, kind


def check_hull(probes, V, what, lengths, tie=False, chunks=(1, 2, 3, 4)):
    """returns {list length: settled rows} and the number of rows refused for a list of more than HL_ROW_MAX entries"""
    H = probes.hull(V)
    try:
        g1, g2, rb, kind = cases(probes, H, V, lengths, tie)
        ref = H.pairs("fused", g1, g2, rb)
        cells = probes.first_cell(g1, g2)
        assert np.all(cells >= 0), what
        cnt = np.diff(H.off.astype(np.int64))[cells]
        served = (cnt >= 1) & (cnt <= list_rows.HL_ROW_MAX)
        first = None
        for chunk in chunks:
            got = probes.list_rows(H, chunk, g1, g2, rb)
            assert np.array_equal(got[0] >= 0, served), f"{what} chunk {chunk}: the row pass served other pairs than lists of 1 .. {list_rows.HL_ROW_MAX} entries"
            settled = got[0] == 1
            for i in np.flatnonzero(served):
                k = kind[i]
                assert settled[i] == (k != "box margin out"), f"{what} chunk {chunk} pair {i} ({k}, list of {cnt[i]}): settled = {got[0][i]}"
                if k == "box separated":
                    assert int(got[1][i]) == 0, f"{what} chunk {chunk} pair {i}: contacts on a separated pair"
            for i in np.flatnonzero(settled):
                v = int(got[1][i])
                assert v == int(ref[1][i]), f"{what} chunk {chunk} {kind[i]} pair {i}: contact mask {v:#x} != fused {int(ref[1][i]):#x}"
                on = [(v >> q) & 1 == 1 for q in range(devprims.NCPP)]
                same = (np.array_equal(got[2][i].view(np.uint32), ref[2][i].view(np.uint32)) and
                        np.array_equal(got[3][i][on].view(np.uint32), ref[3][i][on].view(np.uint32)) and
                        np.array_equal(got[4][i][on].view(np.uint32), ref[4][i][on].view(np.uint32)))
                assert same, f"{what} chunk {chunk} {kind[i]} pair {i} (list of {cnt[i]}): contacts differ from the fused step's"
            # resting and tilted poses touch down: the comparison above is of real contacts
            for i in np.flatnonzero(settled & np.isin(kind, ("plane rest", "box rest", "plane tilted", "box tilted", "box margin in"))):
                assert int(got[1][i]) & 1, f"{what} chunk {chunk} {kind[i]} pair {i}: no contact"
            if first is None:
                first = got
            else:                                      # the same rows whatever the chunk count
                for a, b in zip(first, got):
                    assert np.array_equal(np.asarray(a).view(np.uint32) if a.dtype == np.float32 else a, np.asarray(b).view(np.uint32) if b.dtype == np.float32 else b), f"{what}: chunk {chunk} differs from chunk {chunks[0]}"
        if 4 in chunks:
            # a wavefront of four with a plane row next to box rows, and a separated, an exact and an unsettled row together
            mixed = [w for w in range(0, len(kind) - 3, 4) if served[w:w + 4].all() and kind[w] == "plane rest"]
            assert mixed, f"{what}: no served wavefront of the four leading poses"
            for w in mixed:
                assert list(kind[w:w + 4]) == list(KINDS[:4]) and list(first[0][w:w + 4]) == [1, 1, 1, 0], (what, w, list(first[0][w:w + 4]))
        hist = {}
        for i in np.flatnonzero(first[0] == 1):
            hist[int(cnt[i])] = hist.get(int(cnt[i]), 0) + 1
        return hist, int(((first[0] == -1) & (cnt > list_rows.HL_ROW_MAX)).sum())
    finally:
        H.close()
