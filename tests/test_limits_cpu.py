"""Host-side proof that the cases of tests/util_limits.py reach the limits they are meant for, so that tests/test_gpu_limits.py
cannot go quietly green when a later change to the layout builder moves a case back inside a limit:

  * LIMIT_CASES: under the case's switches both sides' layouts have the forced workgroup count, more blocks than workgroups
    (pack_blocks then makes whole blocks segments), a segment of more than kLdsEvSlots = 128 slices on both sides (more than 256
    on one side for the three-chunk cases), a ragged last chunk, the expected value layout -- and still encode X;
  * GATHER_CASES: k_update's block split, restated from the inverse index, puts every case beyond kStagePtr / kStageIds."""
import numpy as np
import pytest

import util_limits as U
from util_layout import build_layout, reconstruct


@pytest.mark.parametrize("case", U.LIMIT_CASES, ids=U.LIMIT_IDS)
def test_limit_case_has_segments_longer_than_the_evidence_slots(monkeypatch, case):
    import ccfindr_amd as C
    U.set_switches(monkeypatch, case)
    X = U.case_matrix(case)
    assert X.shape == (case.n, case.m) and (X.sum(axis=0) > 0).all() and (X.sum(axis=1) > 0).all()
    if case.kind == "split":
        assert sorted(X[X > 16382].tolist()) == [16383.0, 16384.0, 100000.0]
    if case.kind == "ones_twos":
        assert np.isin(X, (0.0, 1.0, 2.0)).mean() > 0.99 and (X == 2.0).sum() > 50000
    M = C.CountMatrix(X)
    views = [build_layout(M, side, case.r) for side in (0, 1)]
    longest, ragged = [], 0
    for side, v in enumerate(views):
        assert v["side"] == side and v["n_wg"] == case.nwg, (side, v["n_wg"])
        assert v["n_blocks"] > v["n_wg"] and v["n_segs"] == v["n_blocks"], (side, v["n_blocks"], v["n_segs"])
        assert v["wide"] == int(case.kind == "noninteger") and v["max_len"] == case.max_len
        lens = U.segment_lengths(v)
        print(U.case_id(case), "side", side, "slices per segment", int(lens.min()), "-", int(lens.max()))
        longest.append(int(lens.max()))
        ragged += int((lens % U.LDS_EV_SLOTS != 0).sum())
        # (a list of more than 1 023 slices would not fit take_ticket_ends's 10-bit counts either way: not these cases)
        assert np.array_equal(reconstruct(v), X if side == 0 else X.T), side
    assert min(longest) > U.LDS_EV_SLOTS, longest                   # both sides pull at least one list in more than one chunk
    assert (max(longest) - 1) // U.LDS_EV_SLOTS + 1 == case.chunks, (longest, case.chunks)
    if case.chunks == 3:
        assert max(longest) > 2 * U.LDS_EV_SLOTS, longest
    assert ragged > 0                                               # a last chunk shorter than the slots
    M.close()


def test_limit_cases_cover_the_ticket_modes_layouts_and_lane_shares():
    import ccfindr_amd as C
    pads = {C.engine.padded_rank(c.r) for c in U.LIMIT_CASES}
    assert any(R < 8 for R in pads) and any(8 <= R < 16 for R in pads) and any(R >= 16 for R in pads)   # sweep_side_args
    assert {c.kind for c in U.LIMIT_CASES} == {"counts", "noninteger", "split", "ones_twos"}
    assert any(R <= 32 for R in pads) and any(32 < R <= 64 for R in pads) and any(R > 64 for R in pads)  # lane shares 1, 2, 4
    assert {c.chunks for c in U.LIMIT_CASES} == {2, 3}


@pytest.mark.parametrize("g", U.GATHER_CASES, ids=U.GATHER_IDS)
def test_gather_case_is_beyond_what_an_update_block_stages(monkeypatch, g):
    import ccfindr_amd as C
    U.set_gather_switches(monkeypatch, g)
    M = C.CountMatrix(U.gather_matrix(g.name))
    ub = g.grid[1]
    views = [build_layout(M, side, g.r) for side in (0, 1)]
    split = [U.block_split(v, ub) for v in views]
    print(g.name, g.r, "(majors, ids) per block: gene side", split[0], "cell side", split[1])
    for v in views:
        assert v["n_wg"] == g.grid[0]
        assert v["n_tasks"] >= 256 * ub                              # engine.hip stage_ids(): staging is asked for at all
    if g.name == "A":                                               # the id limit alone
        for side in (0, 1):
            (majors, ids), = split[side]
            assert majors < U.STAGE_PTR and ids > U.STAGE_IDS, (side, majors, ids)
    elif g.name == "B":                                             # both kinds of block in the gene side's launch
        staged = [U.block_is_staged(*b) for b in split[0]]
        assert all(majors < U.STAGE_PTR for majors, _ in split[0])
        assert any(ids > U.STAGE_IDS for _, ids in split[0]) and any(staged) and not all(staged), split[0]
    else:                                                           # the pointer limit, with few ids
        assert all(majors >= U.STAGE_PTR and ids <= U.STAGE_IDS for majors, ids in split[1]), split[1]
        assert all(U.block_is_staged(*b) for b in split[0]), split[0]
    M.close()
