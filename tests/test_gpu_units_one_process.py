"""Every translation unit of the library in ONE process: a call into each of qc.hip, gsea.hip, tsne.hip, project.hip,
cophenet.hip, engine.hip and the units on the engine (mlnmf.hip, svd.hip, labels.hip, batch.hip, the stateless form of
stateless.cpp), twice, with vbnmf_pool_trim() (device.hip) between the rounds.  The units share one device buffer
pool and each brings its own code object; the second round runs on buffers the first one gave back to the pool and then to the
driver.  Shapes are the smallest that still reach each kernel.

Round two equals round one bit for bit (the kernels' summation orders are fixed), and round one meets each feature's own
restatement under the bound of that feature's own test:
  gene statistics   tests/util_qc.py: nnz, integer sums and has_mode exactly, ss within SS_BOUND (tests/test_gpu_qc.py)
  GSEA              tests/util_annot.py, assign_dense: the same bits (tests/test_gpu_annot.py)
  t-SNE             tests/util_tsne.py: beta and trips of the unflagged rows exactly; three iterations inside update_bounds
                    (tests/test_gpu_tsne.py, test_step_by_step)
  project           tests/util_project.py: one step, H 1e-12, cell likelihoods 1e-10 (tests/test_gpu_project.py)
  vb_project        tests/util_vb_project.py: one step, lh / eh / dh 1e-12, cell evidences 1e-10 (tests/test_gpu_vb_project.py)
  cophenetic        the host form within TOL of tests/test_gpu_cophenetic_device.py
  resident engine   one step against the CPU oracle, evidence 1e-10 (as smoke())
  ML-NMF            one nmf_update against oracle/mlnmf_oracle.py: w, h 1e-12, likelihood 1e-10 (as smoke())
  truncated SVD     vb_init(initializer='svd2') on the device against numpy's SVD, 1e-6 of the largest entry, and no host-QR form
                    (tests/test_gpu_spmm_svd.py, whose matrix it is at this test's shape: the bound is that of a spectrum with
                    a gap behind the rank -- here sigma_4 / sigma_3 = 0.38 -- which 50 x 30 Poisson noise alone does not have)
  consensus         two label rows from one engine: its cluster_ids, and numpy's integer sums exactly (tests/test_gpu_consensus.py)
  batch             two engines, Itmax = 1: each engine's stand-alone run bit for bit (tests/test_gpu_batch_run.py)
  stateless form    one vbnmf_update against the CPU oracle: the six arrays 1e-12, evidence 1e-10 (as smoke())
On a machine with two devices, a call made for device 1 while device 0 is current must leave device 0 current.
"""
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

import util_annot as UA
import util_project as UP
import util_qc as UQ
import util_tsne as UT
import util_vb_project as UV
from test_gpu_cophenetic_device import TOL as COPH_TOL
from test_gpu_spmm_svd import planted
from util_consensus import groups_of, integer_sums, random_labels

pytestmark = pytest.mark.gpu

R = 3
HY = {"aw": 1.0, "bw": 1.0, "ah": 1.0, "bh": 1.0}
HY_SVD = {"aw": 1.0, "bw": 1.0, "ah": 1.0, "bh": 0.7}
SCH = dict(stop_lying_iter=3, mom_switch_iter=3)


def relerr(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def inputs():
    rng = np.random.default_rng(17)
    d = {}
    d["qc"] = UQ.many_genes(40, m=30, seed=3)
    # GSEA: 50 rows, two clusters, one set, the identity and three more permutations
    names = np.array(["g%d" % i for i in range(50)])
    d["gene"] = np.stack([names[rng.permutation(50)] for _ in range(2)], axis=1).astype(str)
    d["w"] = np.stack([np.sort(np.round(rng.gamma(0.8, 1.0, size=50), 1) + 0.1)[::-1] for _ in range(2)], axis=1)
    d["gset"] = {"s": list(names[5:12])}
    d["perms"] = np.array([np.arange(50)] + [rng.permutation(50) for _ in range(3)], dtype=np.int32)
    d["tsne"] = UT.case(40, 2)
    # 30 new cells on a basis of 50 genes at rank 3; no empty column
    X = rng.poisson(0.6, size=(50, 30)).astype(np.float64)
    X[rng.integers(0, 50, 30), np.arange(30)] += 1
    d["X"] = np.asfortranarray(X)
    d["w_ml"] = rng.uniform(0.1, 1.0, size=(50, R))
    d["h0"] = UP.default_start(X, d["w_ml"])
    alw, bew = rng.uniform(0.5, 6.0, size=(50, R)), rng.uniform(0.02, 0.3, size=(50, R))
    from scipy.special import digamma
    d["ew"], d["lw"] = alw * bew, np.exp(digamma(alw)) * bew
    d["lh0"] = UV.default_start(X, d["ew"])
    d["tuples"], d["sizes"] = groups_of(random_labels(3, 30, 3, seed=5))
    # the units on the engine, at the same 50 x 30 and rank 3
    from ccfindr_amd import synth
    d["w0"], d["h0_ml"] = rng.uniform(size=(50, R)), rng.uniform(size=(R, 30))
    d["Xsvd"] = planted(50, 30, R, seed=7)
    d["whs"] = [synth.random_state(50, 30, R, HY, seed=2001 + b) for b in range(2)]
    return d


def run_alone(M, wh):
    """One device-driven step of a fresh engine -> (the run's result, its lw)."""
    import ccfindr_amd as C
    eng = C.VBEngine(M, R)
    eng.set_state(wh["lw"], wh["lh"], wh["eh"])
    res = eng.run(HY, Itmax=1, history=True)
    lw = eng.get_state(("lw",))["lw"]
    eng.close()
    return res, lw


def one_round(d):
    """A call into every unit -> dict of arrays."""
    import ccfindr_amd as C
    from ccfindr_amd import qc as Q
    from ccfindr_amd import synth
    from ccfindr_amd import bayesian
    P = importlib.import_module("ccfindr_amd.project")
    out = {}
    st = Q.gene_stats(sp.csc_matrix(d["qc"]))
    out.update(qc_nnz=st.ncexpr, qc_sum=st.sum, qc_ss=st.ss, qc_mode=st.mode)
    meta = C.MetaTable(gene=d["gene"], w=d["w"], cv=np.full(d["w"].shape, 0.1))
    a = C.assign_celltype(meta, 2, d["gset"], p=1, p_value=True, perms=d["perms"], return_null=True)
    out.update(gsea_es=a["ES"], gsea_null=a["null_es"], gsea_exceed=a["exceed"])
    c = d["tsne"]
    with C.TSNE(c["X"], perplexity=5.0, normalize=True) as h:
        out.update(tsne_beta=h.beta, tsne_trips=h.trips, tsne_sum_p=h.sum_p)
        h.set_state(UT.start(40, 5))
        for it in range(1, 4):
            f = h.forces(UT.schedule(it, **SCH)[0])
            h.run(1, first_iter=it, **SCH)
            Y, uY, g = h.state()
            out.update({f"tsne_A{it}": f["A"], f"tsne_R{it}": f["R"], f"tsne_z{it}": f["z"], f"tsne_Y{it}": Y, f"tsne_uY{it}": uY,
                        f"tsne_g{it}": g})
    M = C.CountMatrix(d["X"])
    H, lk, _, _ = P.project_columns(M, d["w_ml"], d["h0"].copy(), 0, 30, Itmax=1)
    out.update(proj_h=H, proj_lk=lk)
    lh, eh, dh, ev, _, _ = P.vb_project_columns(M, d["lw"], d["ew"], d["lh0"].copy(), 1.0, 1.0, 0, 30, Itmax=1)
    out.update(vbp_lh=lh, vbp_eh=eh, vbp_dh=dh, vbp_ev=ev)
    M.close()
    out["coph"] = np.array([C.cophenetic_grouped(d["tuples"], d["sizes"], "average", device=0)])
    Xs = synth.drop_empty(synth.simulate_data(200, (100, 150, 250), seed=1, sparse=False))
    hyper = {"aw": 1.0, "bw": 1.0, "ah": 1.0, "bh": 1.0}
    wh = synth.random_state(*Xs.shape, R, hyper, seed=1001)
    eng = C.VBEngine(C.CountMatrix(Xs), R)
    eng.set_state(wh["lw"], wh["lh"], wh["eh"])
    lkh, _ = eng.step(hyper)
    st = eng.get_state(("lw", "lh"))
    eng.close()
    out.update(eng_lkh=np.array([lkh]), eng_lw=st["lw"], eng_lh=st["lh"], eng_X=Xs, eng_wh=wh)
    # mlnmf.hip through the stateless ML form, svd.hip through the svd2 initialiser, the stateless VB form
    ml = C.nmf_update(d["X"], d["w0"], d["h0_ml"])
    out.update(ml_ew=ml["ew"], ml_eh=ml["eh"], ml_lk=np.array([ml["lk"]]))
    init = bayesian.vb_init(50, 30, sp.csc_matrix(d["Xsvd"]), R, HY_SVD, "svd2")
    out.update(svd_lw=init["lw"], svd_lh=init["lh"])
    sl = C.vbnmf_update(d["X"], d["whs"][0], HY, C.EPS)
    out.update({"sl_" + k: sl[k] for k in ("lw", "lh", "ew", "eh", "dw", "dh")}, sl_lkh=np.array([sl["lkh"]]))
    # batch.hip: two engines, one step; labels.hip: two label rows from the first of them, around a host-stepped step
    M = C.CountMatrix(d["X"])
    engs = [C.VBEngine(M, R) for _ in range(2)]
    for e, wh2 in zip(engs, d["whs"]):
        e.set_state(wh2["lw"], wh2["lh"], wh2["eh"])
    got = C.run_batch(engs, [HY, HY], Itmax=1, history=True)
    for b in range(2):
        out.update({f"batch_hist{b}": got[b]["history"], f"batch_lw{b}": engs[b].get_state(("lw",))["lw"]})
        out[f"batch_end{b}"] = np.array([got[b]["it"], got[b]["reason"], got[b]["lk0"], got[b]["lkh"]] + list(got[b]["hyper"].values()))
    cons = C.Consensus(30, R, 2)
    rows = []
    for _ in range(2):
        cons.add(engs[0])
        rows.append(engs[0].cluster_ids())
        engs[0].step(HY)
    s = cons.sums()
    out.update(cons_l0=cons.labels(0), cons_l1=cons.labels(1), cons_ids=np.array(rows),
               cons_sums=np.array([s["runs"], s["s1"], s["s2"], int(s["unlabelled"])], dtype=np.int64), cons_disp=np.array([cons.dispersion()]))
    cons.close()
    for e in engs:
        e.close()
    for b in range(2):                                             # the same engines alone
        res, lw = run_alone(M, d["whs"][b])
        out.update({f"alone_hist{b}": res["history"], f"alone_lw{b}": lw})
        out[f"alone_end{b}"] = np.array([res["it"], res["reason"], res["lk0"], res["lkh"]] + list(res["hyper"].values()))
    M.close()
    return out


def test_every_unit_twice_in_one_process(monkeypatch):
    import ccfindr_amd as C
    from ccfindr_amd.engine import VBEngine
    from oracle import mlnmf_oracle as OM
    from oracle import vbnmf_oracle as O
    spmm_calls, spmm = [], VBEngine.spmm                 # (the host-QR form of the truncated SVD goes through VBEngine.spmm)
    monkeypatch.setattr(VBEngine, "spmm", lambda self, B, transpose=False: (spmm_calls.append(1), spmm(self, B, transpose=transpose))[1])
    d = inputs()
    first = one_round(d)
    C.load().vbnmf_pool_trim()
    second = one_round(d)
    Xs, wh = first.pop("eng_X"), first.pop("eng_wh")
    second.pop("eng_X"), second.pop("eng_wh")
    for k in first:
        a, b = np.ascontiguousarray(first[k]), np.ascontiguousarray(second[k])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k

    # gene statistics
    nnz, s, ss, mode = UQ.dense_stats(d["qc"])
    assert np.array_equal(first["qc_nnz"], nnz) and np.array_equal(first["qc_sum"], s) and np.array_equal(first["qc_mode"], mode)
    for i, row in enumerate(d["qc"]):
        rs, rss = UQ.row_errors(row[row != 0], 30, first["qc_sum"][i], first["qc_ss"][i])
        assert rs == 0.0 and rss <= UQ.SS_BOUND, (i, rs, rss)
    # GSEA
    from ccfindr_amd import annotate as A
    meta = C.MetaTable(gene=d["gene"], w=d["w"], cv=np.full(d["w"].shape, 0.1))
    tb = A.gsea_tables(meta, d["gset"], p=1, grp_prefix=("IG",))
    es, exceed, null = UA.assign_dense(meta.gene, meta.w, tb["wp"].T, d["gset"], d["perms"], ("IG",))
    assert UA.bits_equal(first["gsea_es"], es) and UA.bits_equal(first["gsea_null"], null)
    assert np.array_equal(first["gsea_exceed"], exceed)
    # t-SNE: the affinities, then each of the three iterations from the device's own state before it
    c = d["tsne"]
    beta, S, trips, flagged = UT.affinities(c["Xn"], 5.0)
    assert flagged.sum() <= 0.01 * 40
    assert np.all(((first["tsne_beta"] == beta) & (first["tsne_trips"] == trips)) | flagged)
    Y, uY, g = UT.start(40, 5), np.zeros((40, 2)), np.ones((40, 2))
    inside = total = 0
    for it in range(1, 4):
        m = UT.schedule(it, **SCH)[1]
        A_, R_, z_ = first[f"tsne_A{it}"], first[f"tsne_R{it}"], first[f"tsne_z{it}"]
        wY, wuY, wg, _ = UT.update(Y, uY, g, A_, R_, z_, m)
        ub = UT.update_bounds(Y, uY, g, A_, R_, z_, m)
        either = np.abs(ub["dY"]) <= ub["bdY"]              # may have taken the other gain: left out, and counted
        inside += int(either.sum())
        total += either.size
        ok = ~either
        Y, uY, g = first[f"tsne_Y{it}"], first[f"tsne_uY{it}"], first[f"tsne_g{it}"]
        assert np.all(np.abs(g - wg)[ok] <= ub["bgain"][ok]) and np.all(np.abs(uY - wuY)[ok] <= 2 * ub["buY"][ok]), it
        rows = ok.all(axis=1)
        assert np.all(np.abs(Y - wY)[rows] <= 2 * ub["bY"][rows]), it
    assert inside <= 0.01 * total
    # project and vb_project, one step
    want = UP.h_half(d["X"], d["w_ml"], d["h0"])
    assert relerr(first["proj_h"], want) <= 1e-12
    assert relerr(first["proj_lk"], UP.cell_likelihood(d["X"], d["w_ml"], want)) <= 1e-10
    cew = d["ew"].sum(axis=0)
    wl, we, wd, alh = UV.h_half(d["X"], d["lw"], cew, d["lh0"], 1.0, 1.0)
    for k, w_ in (("vbp_lh", wl), ("vbp_eh", we), ("vbp_dh", wd)):
        assert relerr(first[k], w_) <= 1e-12, k
    assert relerr(first["vbp_ev"], UV.cell_evidence(d["X"], d["lw"], cew, wl, we, alh, 1.0, 1.0)) <= 1e-10
    # cophenetic
    host = C.cophenetic_grouped(d["tuples"], d["sizes"], "average")
    assert abs(first["coph"][0] - host) <= COPH_TOL, (first["coph"][0], host)
    # resident engine
    ref = O.update_dense(Xs, wh, HY, C.EPS)
    assert abs(first["eng_lkh"][0] / ref["lkh"] - 1) < 1e-10
    # ML-NMF, one step
    mo = OM.nmf_update_literal(d["X"], d["w0"], d["h0_ml"])
    assert relerr(first["ml_ew"], mo["ew"]) < 1e-12 and relerr(first["ml_eh"], mo["eh"]) < 1e-12
    assert abs(first["ml_lk"][0] / OM.likelihood_literal(d["X"], mo["ew"], mo["eh"]) - 1) < 1e-10
    # the svd2 initialiser: the device-resident SVD's triplets, not the host-QR form's
    assert not spmm_calls
    U, D, Vt = np.linalg.svd(d["Xsvd"], full_matrices=False)
    w, h = np.abs(U[:, :R]), np.abs(np.diag(D[:R]) @ Vt[:R])
    scale = HY_SVD["bh"] / np.mean(h)
    print("svd2: lw", np.max(np.abs(first["svd_lw"] - w / scale)) / np.max(w / scale), "lh", np.max(np.abs(first["svd_lh"] - h * scale)) / np.max(h * scale))
    assert np.max(np.abs(first["svd_lw"] - w / scale)) <= 1e-6 * np.max(w / scale)
    assert np.max(np.abs(first["svd_lh"] - h * scale)) <= 1e-6 * np.max(h * scale)
    assert np.mean(first["svd_lh"]) == pytest.approx(HY_SVD["bh"])
    # the stateless form
    ref = O.update_dense(d["X"], d["whs"][0], HY, C.EPS)
    for k in ("lw", "lh", "ew", "eh", "dw", "dh"):
        assert relerr(first["sl_" + k], ref[k]) < 1e-12, k
    assert abs(first["sl_lkh"][0] / ref["lkh"] - 1) < 1e-10
    # the batch: each engine as alone
    for b in range(2):
        assert first[f"batch_end{b}"][0] == 1
        for k in ("hist", "lw", "end"):
            assert np.array_equal(first[f"batch_{k}{b}"], first[f"alone_{k}{b}"], equal_nan=True), (k, b)
    # the consensus accumulator
    assert np.array_equal(first["cons_l0"], first["cons_ids"][0]) and np.array_equal(first["cons_l1"], first["cons_ids"][1])
    assert tuple(first["cons_sums"]) == (2,) + integer_sums(first["cons_ids"], R) + (0,)

    # a call made for device 1 while device 0 is current leaves device 0 current (where there are two devices)
    import torch
    if torch.cuda.device_count() >= 2:
        from ccfindr_amd import qc as Q
        torch.cuda.set_device(0)
        st = Q.gene_stats(sp.csc_matrix(d["qc"]), device=1)
        assert torch.cuda.current_device() == 0
        assert st.ss.tobytes() == np.ascontiguousarray(first["qc_ss"]).tobytes()
