"""The committed case list of the option sweep (tests/util_configs.py) on the CPU: it covers what the sweep promises, every case
is drawn as its seed says, and every case's layouts -- cut under its own switches, rank geometry, grid and columns -- encode
exactly its matrix (tests/util_layout.py reconstruct, with the structural checks of both leading stretches).  Also holds the
numpy restatement of the device's Philox4x32-10 (tests/util_philox.py) to the generator's published answers."""
import numpy as np
import pytest

import util_configs as U
from util_layout import build_layout, reconstruct


def _covered(key):
    return {key(c) for c in U.CASES}


def test_the_case_list_covers_the_required_tuples():
    assert _covered(lambda c: c["width"] if c["path"] in U.VB_PATHS else None) >= set(U.PADDED_WIDTHS)
    assert _covered(lambda c: (U.lane_share(c["width"]), U.layout_of(c["kind"]))) >= {
        (sp, lay) for sp in (1, 2, 4) for lay in ("packed", "wide", "split")}
    assert _covered(lambda c: (c["path"], c["order"])) >= {(p, o) for p in U.PATHS for o in (0, 1)}
    kind_of_path = lambda p: "ml" if p in U.ML_PATHS else p
    assert _covered(lambda c: (c["forced"], kind_of_path(c["path"]))) >= {
        (f, p) for f in U.FORCED for p in ("batch", "group", "ml")}
    assert _covered(lambda c: (c["fudge"], c["path"])) >= {(f, p) for f in (0.0, 1e-3) for p in ("run", "batch")}
    assert _covered(lambda c: (c["kind"], c["path"] in U.ML_PATHS)) >= {(k, ml) for k in U.STRETCH_KINDS for ml in (False, True)}
    # ... and every pinned requirement is met by the case drawn for it
    for (what, pins), c in zip(U.REQUIRED, U.CASES):
        for k, v in pins.items():
            assert c[k] == v, (what, pins, U.case_id(c))


def test_draws_are_a_function_of_the_seed_and_respect_the_api():
    for seed in range(200):
        c = U.draw_config(seed)
        assert c == U.draw_config(seed)
        assert np.array_equal(U.case_matrix(c), U.case_matrix(U.draw_config(seed)))
        assert 1 <= c["rank"] <= 128 and U.padded_rank(c["rank"]) <= c["width"] and c["width"] in U.PADDED_WIDTHS
        if c["path"] in U.BATCH_PATHS:
            assert c["width"] <= U.BATCH_MAX_WIDTH and c["pad_rank"] == c["width"] and c["grid"] is not None
            assert len(c["ranks"]) == c["B"] and all(1 <= r <= c["width"] for r in c["ranks"])
        if c["path"] == "group":
            assert c["pad_rank"] is None and c["grid"] is None and c["geometry_rank"] is None
            cuts = c["cuts"]
            assert cuts[0][0] == 0 and cuts[-1][1] == c["m"] and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
            assert len(cuts) == c["P"] and min(e - b for b, e in cuts) == 1
        if c["path"] in U.ML_PATHS:
            assert c["fudge"] == U.EPS
    assert len({U.case_id(c) for c in U.CASES}) == len(U.CASES)


def _nwg(c):
    """The sweep workgroups of the case's engines (engine.hip: a forced count, capped by the grid's)."""
    nwg = c["forced"][1] if c["forced"] else 256
    return min(nwg, c["grid"][0]) if c["grid"] else nwg


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_every_case_layout_encodes_its_matrix(case):
    import ccfindr_amd as C
    X = U.case_matrix(case)
    env = dict(U.case_env(case), VBNMF_NWG=str(_nwg(case)))
    with U.switches(env):
        M = C.CountMatrix(X)
        try:
            for cols in case.get("cuts") or [None]:
                b, e = cols if cols else (0, X.shape[1])
                for side in (0, 1):
                    v = build_layout(M, side, U.layout_rank(case), cols)
                    assert v["n_wg"] == _nwg(case) and v["wide"] == int(case["kind"] == "noninteger"), U.case_id(case)
                    want = X[:, b:e] if side == 0 else X[:, b:e].T
                    assert np.array_equal(reconstruct(v), want), (U.case_id(case), cols, side)
        finally:
            M.close()


# ---- the restatement of the device's generator -------------------------------------------------------------------------------
def test_philox_restatement_gives_the_published_answers():
    """Philox4x32-10 known answers (Salmon et al., SC'11; Random123's kat_vectors)."""
    from util_philox import philox4x32
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = philox4x32(*[np.array([v]) for v in ctr], *key)
        assert tuple(int(g[0]) for g in got) == want, (ctr, key)


@pytest.mark.parametrize("a", [0.05, 0.3, 1.0, 12.0])
def test_gamma_restatement_has_the_gamma_distribution(a):
    from scipy import stats
    from util_philox import gamma_draws
    x = gamma_draws(a, 2.0 / a, np.arange(20000), 1, 0x9E3779B97F4A7C15)
    ks = stats.kstest(x[x > 0], stats.gamma(a, scale=2.0 / a).cdf)
    assert ks.pvalue > 1e-3, ks
    assert abs(x.mean() / 2.0 - 1) < 5.0 / np.sqrt(a * x.size)
