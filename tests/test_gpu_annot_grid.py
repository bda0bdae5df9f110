"""k_gsea_perm / k_gsea_count (csrc/gsea.h) where tests/test_gpu_annot.py does not take them: a workgroup that goes round its
item loop more than once, the prefix scan of the validity words past its first wave (N > 4096) and with several words a thread
(N > 16384), k_gsea_count past its first workgroup, rank 128 and a chunk of one permutation.  The reference is the same as there --
the dense restatement of R/gsea.R:41-128 (tests/util_annot.py, compare): ES, the null scores and the p-values equal in bits and
NaN positions, the exceed counts as integers; there is no tolerance to set.  The inputs come from util_annot.grid_case;
tests/test_annot_grid_cpu.py shows without a device that they are what the docstrings here say.

k_gsea_perm runs on min(items, CUs x 8) workgroups (gsea.hip, gsea_grid), where items = the permutations of one chunk x the rank.
The library does not report that grid; grid_workgroups() forms it as tests/test_gpu_project.py does, and every test that needs
more items than workgroups asserts it, so that on a larger part it fails instead of testing nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_annot as U  # noqa: E402

import ccfindr_amd as C  # noqa: E402
from ccfindr_amd import annotate as A  # noqa: E402

pytestmark = pytest.mark.gpu

INFO = A.gsea_info()
W, G, CAP = INFO["wave_width"], INFO["workgroup_size"], INFO["max_set_hits"]


def grid_workgroups():
    """Workgroups of k_gsea_perm's grid when the items allow: as many as the CUs hold threads for (gsea.hip, gsea_grid: CUs x 2048 / 256)."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8


def run(name):
    c = U.grid_case(name)
    return c, U.compare(c["meta"], c["gset"], c["p"], c["perms"], c["label"])


def test_default_nperm_takes_several_items_per_workgroup():
    """assign_celltype's default nperm = 1000, as explicit perms (the identity and a repeated row among them): N = 130, r = 5,
    p = 0.5, 5000 items in one launch, more than twice the grid.  Clusters 1 and 3 end in NA rows; the grid's 2048 workgroups
    are 3 mod 5, so a workgroup's successive items are different clusters: its scratch words and prefix are rewritten for another
    cluster's rows, and it passes from a cluster with NA rows to one without and back.  Five sets: none, 1, W, W + 1 genes and the
    prefix set."""
    c = U.grid_case("default")
    n, r = c["meta"].gene.shape
    assert (n, r, len(c["perms"]), len(c["gset"])) == (130, 5, 1000, 5)
    assert U.launch_items(n, 1000, r) == 1000 * r > 2 * grid_workgroups(), grid_workgroups()
    assert grid_workgroups() % r != 0
    run("default")


def test_rank_128_and_two_workgroups_of_counts():
    """Rank 128 = VBNMF_MAX_RANK, N = 33, 40 permutations: 5120 items, more than twice the grid.  Every fourth cluster has NA rows.
    Three sets (none, 12 genes, the prefix set): nq = 384 scores, so k_gsea_count runs two workgroups, and the second one holds
    the prefix set's counts."""
    c = U.grid_case("rank128")
    n, r = c["meta"].gene.shape
    assert r == 128 and len(c["gset"]) * r == 384 > G
    assert U.launch_items(n, len(c["perms"]), r) == 5120 > 2 * grid_workgroups(), grid_workgroups()
    _, (out, es) = run("rank128")
    assert (out["exceed"].reshape(-1)[G:] > 0).any()


def test_many_sets_six_workgroups_of_counts():
    """300 sets of 1 .. 12 genes at N = 40, r = 5: nq = 1500, six workgroups of k_gsea_count, 8 permutations.  At most a quarter of
    the observed scores are NaN, and the counts take at least three values."""
    c = U.grid_case("many_sets")
    assert len(c["gset"]) * c["meta"].rank == 1500 > 5 * G
    _, (out, es) = run("many_sets")
    assert np.isnan(es).sum() <= es.size // 4 and len(set(out["exceed"].reshape(-1).tolist())) >= 3
    flat = out["exceed"].reshape(-1)
    assert all((flat[q:q + G] > 0).any() for q in range(0, flat.size, G))


@pytest.mark.parametrize("n,r", U.LONG_SIZES)
def test_prefix_scan_past_its_first_wave(n, r):
    """Tables of more than 4096 rows with NA rows (util_annot._long_table).  N = 4200: nW = 66 validity words, threads 64 and 65 --
    wave 1 -- own one each and take wave 0's total through LDS.  N = 16500: nW = 258, two words a thread, thread 128 owns the last
    two.  N = 16440: nW = 257, thread 128's stretch is cut to one word.  Cluster 0 has no NA rows; the last cluster has 400 NA
    rows from row 3000 on and 30 at its end, so the observed scores too rank hits from wave 1's words; at r = 3 cluster 1 is NA
    from row 4000 on.  Sets of 1, W + 1 and 300 genes, the prefix set (a tenth of the rows), none, and `placed`: hits in the last
    cluster at the last position of words 0 and 64 per - 1, the first position of word 64 per -- the first that thread 64 owns
    -- and the last valid row.  6 permutations."""
    nw, per, first = U.scan_shape(n)
    assert nw > W and (per > 1) == (n > W * W * 4) and first == W * W * per
    run("rows%d" % n)


def test_chunk_of_one_permutation(monkeypatch):
    """VBNMF_GSEA_CHUNK_PERMS = 1 at N = 257, r = 3: a grid of 3 workgroups, one launch of both kernels per permutation, the
    counts added over five launches."""
    monkeypatch.setenv("VBNMF_GSEA_CHUNK_PERMS", "1")
    c = U.grid_case("chunk1")
    assert A.gsea_info(257)["chunk_perms"] == 1 and c["meta"].gene.shape == (257, 3) and len(c["perms"]) == 5
    run("chunk1")


def _call(c, perms):
    return C.assign_celltype(c["meta"], c["meta"].rank, c["gset"], p=c["p"], p_value=True, perms=perms, grp_prefix=("IG",), return_null=True)


@pytest.mark.parametrize("r", (3, 10))
def test_several_items_per_workgroup_against_one(monkeypatch, r):
    """N = 20 000 with NA clusters, 1000 seeded permutations, no reference: the call as it stands against the same call with
    VBNMF_GSEA_CHUNK_PERMS = 64 -- 64 r items a launch, every item alone on its workgroup, the path that the dense form pins at
    N = 4096 (tests/test_gpu_annot.py) -- and against its two halves of perms, null scores concatenated and counts added.

    At N = 20 000 a chunk is 419 permutations (64 MB / 8N).  At rank 10 the call as it stands launches 4190 items, more than twice
    the grid, and this is the multi-item path at a realistic size.  At rank 3 a launch has 1257 items, fewer than the grid has
    workgroups, so no workgroup takes a second one whatever nperm is: that case holds the three chunkings (419, 64 and
    419 + 81 twice) to the same bits and says nothing about the item loop."""
    c = U.grid_case("wide%d" % r)
    n, nperm = c["meta"].gene.shape[0], len(c["perms"])
    assert (n, nperm) == (20000, 1000) and A.gsea_info(n)["chunk_perms"] == 419
    if r == 10:
        assert U.launch_items(n, nperm, r) == 4190 > 2 * grid_workgroups(), grid_workgroups()
    whole = _call(c, c["perms"])
    halves = [_call(c, c["perms"][:nperm // 2]), _call(c, c["perms"][nperm // 2:])]
    monkeypatch.setenv("VBNMF_GSEA_CHUNK_PERMS", "64")
    assert A.gsea_info(n)["chunk_perms"] == 64 and 64 * r <= grid_workgroups()
    alone = _call(c, c["perms"])
    nan = np.isnan(whole["ES"])
    sets = list(c["gset"])
    assert nan[sets.index("none")].all() and nan.sum() == r
    print(f"N={n} r={r}: {int(nan.sum())} of {nan.size} scores NaN, exceed in [{whole['exceed'].min()}, {whole['exceed'].max()}]")
    for other in [alone] + halves:
        assert U.bits_equal(other["ES"], whole["ES"])
    assert U.bits_equal(alone["null_es"], whole["null_es"]) and np.array_equal(alone["exceed"], whole["exceed"])
    assert U.bits_equal(np.concatenate([h["null_es"] for h in halves]), whole["null_es"])
    assert np.array_equal(np.where(nan, -1, halves[0]["exceed"] + halves[1]["exceed"]), whole["exceed"])
    assert U.bits_equal(whole["null_es"][0], whole["ES"]) and U.bits_equal(whole["null_es"][1], whole["null_es"][2])
    inner = whole["exceed"][(whole["exceed"] > 0) & (whole["exceed"] < nperm)]
    assert len(set(inner.tolist())) > 1
