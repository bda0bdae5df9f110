"""Merged pieces in the layout (host only): the pieces of a cut (major, block) pair sit in consecutive lanes, the row index
names the first lane of every run, and the blob carries both."""
import numpy as np
import pytest

from util_layout import build_layout, reconstruct
from util_piece_merge import IDLE, layout_view, matrix_300x700, matrix_64x3000, runs_of, set_geometry

MATRICES = {"300x700": matrix_300x700, "64x3000": matrix_64x3000}


def _pairs_and_straddles(v):
    """Non-empty (major, block) pairs of a layout and, per pair, the slices it touches beyond its first."""
    tm = v["task_major"].reshape(-1, 64)
    slices_of = {}
    for s in range(tm.shape[0]):
        for M in np.unique(tm[s][tm[s] != IDLE]):
            slices_of.setdefault((int(M), int(v["slice_block"][s])), []).append(s)
    return len(slices_of), sum(len(q) - 1 for q in slices_of.values()), slices_of


@pytest.mark.parametrize("name", sorted(MATRICES))
@pytest.mark.parametrize("r", [3, 10])
def test_groups_and_row_index(monkeypatch, name, r):
    import ccfindr_amd as C
    set_geometry(monkeypatch, r)
    X = MATRICES[name]()
    M = C.CountMatrix(X)
    for side in (0, 1):
        assert np.array_equal(reconstruct(build_layout(M, side, r)), X if side == 0 else X.T)
        v = layout_view(M, side, r)
        assert v["merge"] == 1 and v["max_len"] == 16
        tm = v["task_major"].reshape(-1, 64)
        pieces = np.diff(v["inv_ptr"])
        assert pieces.max() > (64 if (name == "64x3000" and side == 0) else 2)       # pairs cut in 2 ... more than 64 pieces
        # every pair's pieces are consecutive lanes of a slice: ONE run per (pair, slice)
        npairs, nstraddle, slices_of = _pairs_and_straddles(v)
        runs = runs_of(v)
        per_pair_slice = {}
        for s, lane, length, _ in runs:
            key = (int(tm[s, lane]), s)
            assert key not in per_pair_slice, ("the pieces of a pair are apart in slice %d" % s, key)
            per_pair_slice[key] = length
        # ... and a pair of P pieces that begins at lane l fills its slices: only its last slice may hold other tasks behind it
        for (major, blk), ss in slices_of.items():
            lens = sorted(per_pair_slice[(major, s)] for s in ss)
            total = sum(lens)
            assert len(ss) <= (total + 62) // 64 + 1, (major, blk, lens)
        # the row index: exactly the first lane of every run, each once, per major in the inverse index's order
        leaders = np.array(sorted(s * 64 + lane for s, lane, _, _ in runs), dtype=np.int64)
        assert v["n_rows"] == leaders.size == v["row_task"].size
        assert np.array_equal(np.sort(v["row_task"].astype(np.int64)), leaders)
        lead = np.zeros(tm.size, dtype=bool)
        lead[leaders] = True
        for major in range(v["n_major"]):
            inv = v["inv_task"][v["inv_ptr"][major]:v["inv_ptr"][major + 1]]
            rows = v["row_task"][v["row_ptr"][major]:v["row_ptr"][major + 1]]
            assert (v["task_major"][rows] == major).all()
            assert np.array_equal(rows, inv[lead[inv]])
        assert v["n_rows"] <= npairs + nstraddle
        assert v["n_rows"] < v["n_tasks"]
    M.close()


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_merging_off_keeps_one_row_per_task(monkeypatch, name):
    import ccfindr_amd as C
    set_geometry(monkeypatch, 10, merge=0)
    X = MATRICES[name]()
    M = C.CountMatrix(X)
    for side in (0, 1):
        v = layout_view(M, side, 10)
        assert v["merge"] == 0 and v["n_rows"] == v["n_tasks"]
        assert np.array_equal(v["row_ptr"], v["inv_ptr"]) and np.array_equal(v["row_task"], v["inv_task"])
        assert np.array_equal(reconstruct(build_layout(M, side, 10)), X if side == 0 else X.T)
    M.close()


def test_ranks_above_32_are_not_merged(monkeypatch):
    import ccfindr_amd as C
    set_geometry(monkeypatch, 40, merge=1)                       # forcing it on does not reach the shared-task ranks
    M = C.CountMatrix(matrix_300x700())
    v = layout_view(M, 0, 40)
    assert v["merge"] == 0 and np.array_equal(v["row_task"], v["inv_task"])
    M.close()


def _blob_arrays(blob):
    """(header words, byte ranges of the blob's arrays)"""
    h = np.frombuffer(bytes(blob[:56 * 8]), dtype=np.int64)
    off, out = 56 * 8, []
    for q in range(17):
        off = (off + 63) & ~63
        out.append((off, off + int(h[32 + q])))
        off += int(h[32 + q])
    return h, out


def test_blob_round_trip_keeps_the_row_index_and_old_blobs_are_refused(monkeypatch):
    import ccfindr_amd as C
    from ccfindr_amd import _native as N
    set_geometry(monkeypatch, 10)
    M = C.CountMatrix(matrix_300x700())
    S = C.CountMatrix.shell(M.meta())
    for side in (0, 1):
        v = layout_view(M, side, 10)
        nb = M.layout_blob_size(side, 10, 256)
        blob = bytearray(nb)
        assert M.export_layout(side, 10, 256, blob) == nb
        h, ranges = _blob_arrays(blob)
        assert h[1] == 3 and h[25] == v["n_rows"] and h[26] == 1 and v["n_rows"] < v["n_tasks"]
        row_ptr = np.frombuffer(bytes(blob[ranges[15][0]:ranges[15][1]]), dtype=np.int32)
        row_task = np.frombuffer(bytes(blob[ranges[16][0]:ranges[16][1]]), dtype=np.uint32)
        assert np.array_equal(row_ptr, v["row_ptr"]) and np.array_equal(row_task, v["row_task"])
        S.import_layout(blob)
        back = bytearray(nb)
        assert S.export_layout(side, 10, 256, back) == nb and back == blob
        old = bytearray(blob)
        old[8:16] = np.int64(2).tobytes()                         # the version before the row index
        with pytest.raises(N.VBNMFError) as ei:
            S.import_layout(old)
        assert ei.value.code == N.ERR_BAD_ARG
        bad = bytearray(blob)                                     # a row index that names a task outside the layout
        bad[ranges[16][0]:ranges[16][0] + 4] = np.uint32(0x7FFFFFFF).tobytes()
        with pytest.raises(N.VBNMFError):
            S.import_layout(bad)
    S.close(); M.close()
