"""The inputs of tests/test_gpu_annot_grid.py, checked without a device: both files take them from util_annot.grid_case, so what
is shown here holds for what the device computes on.  With the dense form alone (util_annot.grid_dense): the NaN share of every
case, NA and NA-free clusters in every case, observed exceed counts that spread, the largest set of every case, the named hit
positions of the long tables, and -- from vbnmf_gsea_info's constants -- the word and item counts that the device tests' docstrings
state.  The workgroup counts are those of a part with 256 CUs, util_annot.GRID_PART; the device tests assert the real ones."""
import numpy as np
import pytest

import util_annot as U

from ccfindr_amd import annotate as A

INFO = A.gsea_info()
W, G, CAP = INFO["wave_width"], INFO["workgroup_size"], INFO["max_set_hits"]
LONG = tuple("rows%d" % n for n, _ in U.LONG_SIZES)
ALL = U.DENSE_CASES + ("wide3", "wide10")


def _na_clusters(meta):
    return np.flatnonzero(np.isnan(meta.w).any(axis=0))


def _hits(tb, nsets, k, s):
    q = k * nsets + s
    return tb["hit_row"][tb["hit_ptr"][q]:tb["hit_ptr"][q + 1]]


@pytest.mark.parametrize("name", ALL)
def test_na_and_na_free_clusters(name):
    c = U.grid_case(name)
    na = _na_clusters(c["meta"])
    assert 0 < len(na) < c["meta"].rank, (name, na)
    assert not np.isnan(c["meta"].w[0]).any()                          # no cluster is empty
    assert len(c["perms"]) == {"default": 1000, "rank128": 40, "many_sets": 8, "chunk1": 5, "wide3": 1000, "wide10": 1000}.get(name, 6)
    assert np.array_equal(c["perms"][0], np.arange(c["meta"].gene.shape[0])) and np.array_equal(c["perms"][1], c["perms"][2])
    if name.startswith("wide"):
        # no dense form at this size: from the hit counts, every set but `none` has a hit and a miss in every cluster (no NaN)
        tb = A.gsea_tables(c["meta"], c["gset"], p=c["p"], grp_prefix=("IG",))
        T = np.diff(tb["hit_ptr"]).reshape(c["meta"].rank, len(c["gset"]))
        assert list(c["gset"])[0] == "none" and not T[:, 0].any() and T[:, 1:].all() and T.max() <= CAP
        assert T.max() < tb["valid"].sum(axis=1).min()


def test_clusters_are_where_the_docstrings_say():
    assert _na_clusters(U.grid_case("default")["meta"]).tolist() == [1, 3]
    assert _na_clusters(U.grid_case("rank128")["meta"]).tolist() == list(range(3, 128, 4))
    for name in LONG:
        meta = U.grid_case(name)["meta"]
        n, r = meta.gene.shape
        assert (n, r) in U.LONG_SIZES and _na_clusters(meta).tolist() == list(range(1, r))
        for k in _na_clusters(meta):
            assert np.flatnonzero(np.isnan(meta.w[:, k])).min() < CAP, "the NA rows start before row 4096"


def test_item_and_word_counts():
    """What the device tests' docstrings say about the launches, from the library's constants."""
    assert (W, G) == (64, 256)
    c = U.grid_case("default")
    assert c["meta"].gene.shape == (130, 5) and U.launch_items(130, 1000, 5) == 5000 > 2 * U.GRID_PART
    assert U.GRID_PART % 5 == 3                                         # a workgroup's next item is another cluster
    c = U.grid_case("rank128")
    assert c["meta"].gene.shape == (33, 128) and U.launch_items(33, 40, 128) == 5120 > 2 * U.GRID_PART
    assert len(c["gset"]) * 128 == 384 > G
    c = U.grid_case("many_sets")
    assert c["meta"].gene.shape == (40, 5) and len(c["gset"]) * 5 == 1500 > 5 * G
    assert sorted({len(g) for g in c["gset"].values()}) == list(range(1, 13))
    assert U.scan_shape(4200) == (66, 1, 4096)                          # threads 64 and 65, of wave 1, own a word each
    assert U.scan_shape(16500) == (258, 2, 8192)                        # two words a thread; thread 128 owns words 256, 257
    assert U.scan_shape(16440) == (257, 2, 8192)                        # ... thread 128's stretch is cut to word 256
    # N = 20 000: a chunk is 419 permutations, so at rank 3 the largest launch has 1257 items -- fewer than the grid's
    # workgroups: no workgroup takes a second item whatever nperm is.  Rank 10 gives 4190.
    assert A.gsea_info(20000)["chunk_perms"] == 419
    assert U.launch_items(20000, 1000, 3) == 1257 < U.GRID_PART and U.launch_items(20000, 1000, 10) == 4190 > 2 * U.GRID_PART
    assert 64 * 10 <= U.GRID_PART                                       # a chunk of 64: every item alone on its workgroup


@pytest.mark.parametrize("name", U.DENSE_CASES)
def test_dense_scores_of_the_inputs(name):
    c, d = U.grid_case(name), U.grid_dense(name)
    es, exceed, nperm = d["es"], d["exceed"], len(c["perms"])
    sets = list(c["gset"])
    nan = np.isnan(es)
    most = int(np.diff(d["tb"]["hit_ptr"]).max())
    inner = sorted(set(exceed[(exceed > 0) & (exceed < nperm)].tolist()))
    print(f"{name}: dense form {d['seconds']:.2f} s; {int(nan.sum())} of {es.size} observed scores NaN; largest set {most} hits; "
          f"exceed strictly inside (0, {nperm}): {len(inner)} values")
    # NaN
    if name == "many_sets":
        assert nan.sum() <= es.size // 4
        assert len(set(exceed.reshape(-1).tolist())) >= 3
    elif name != "chunk1":                                              # (chunk1 keeps make_sets' `every`, NaN where M = 0)
        assert nan[sets.index("none")].all() and nan.sum() == es.shape[1]
    # exceed
    assert len(inner) > 1, inner
    # k_gsea_count: every workgroup of 256 scores holds one that is finite and was exceeded
    flat = exceed.reshape(-1)
    for q0 in range(0, flat.size, G):
        assert (flat[q0:q0 + G] > 0).any(), (name, q0)
    # the largest set
    valid = ~np.isnan(c["meta"].w)
    count = np.array([[int(U.overlap(c["meta"].gene[valid[:, k], k], gs).sum()) for gs in c["gset"].values()] for k in range(es.shape[1])])
    assert most == count.max() <= CAP
    assert most == {"default": W + 1, "rank128": 12, "many_sets": 12, "rows4200": 422, "rows16500": 1652, "rows16440": 1646, "chunk1": 257}[name]


@pytest.mark.parametrize("name", LONG)
def test_long_tables_have_hits_at_the_named_positions(name):
    """From gsea_tables' hit rows and the valid column, for the set `placed` in the last cluster."""
    c, d = U.grid_case(name), U.grid_dense(name)
    n, r = c["meta"].gene.shape
    nw, per, first = U.scan_shape(n)
    k, s = r - 1, list(c["gset"]).index("placed")
    valid = d["tb"]["valid"][k].astype(bool)
    rows = _hits(d["tb"], len(c["gset"]), k, s)
    assert len(rows) == 4
    last_valid = int(np.flatnonzero(valid).max())
    assert first in rows and first // W == 64 * per                     # the first position of thread 64's first word
    assert last_valid in rows and last_valid // W == nw - 1 and last_valid < n - 1 and not valid[last_valid + 1:].any()
    assert W - 1 in rows and first - 1 in rows                          # bit 63 of words 0 and 64 per - 1
    assert not valid[3000:3400].any() and valid[3400:first + 1].all()   # NA rows before the hits that wave 1's words rank
    # the 300-gene set has hits in words of every wave's stretch in the NA clusters
    s300 = list(c["gset"]).index("size300")
    for kk in range(1, r):
        words = _hits(d["tb"], len(c["gset"]), kk, s300) // W
        owners = {int(w // per) // W for w in words}
        assert 0 in owners and (kk != k or 1 in owners), (kk, owners)
    # every permutation but the identity puts hits of that set behind word 64 per -- ranked from wave 1's words -- in every NA cluster
    for kk in range(1, r):
        rows300 = _hits(d["tb"], len(c["gset"]), kk, s300)
        for perm in c["perms"][1:]:
            assert (np.argsort(perm)[rows300] >= first).any(), kk
