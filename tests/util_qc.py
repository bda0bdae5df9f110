"""The reference's quality-control step restated line by line in numpy, the per-gene sums in 50-digit arithmetic (mpmath),
and the cases the tests run them on -- TEST INFRASTRUCTURE ONLY.

Every function cites the lines of the reference's R/utils.R it restates; all of them work on a dense genes x cells array, as
the reference's own expressions do once ``counts(object)`` is indexed.
"""
import mpmath as mp
import numpy as np

mp.mp.dps = 50

# ---- bounds ------------------------------------------------------------------------------------------------------------------
# The kernel's summation order (csrc/qc.h): entry e of a row belongs to thread e mod 256 (lane e in a short row); a thread adds
# its entries in ascending order; xor butterflies over the 64 lanes; the four waves in order.  A sum of `len` terms therefore
# passes through at most ceil(len / 256) - 1 serial adds, 6 butterfly levels and 3 wave adds: 11 roundings at the longest row
# the tests build (2 P + 1 = 513 entries), so |sum - exact| <= 11 u sum|x| = 1.3e-15 sum|x| (u = 2^-53).
# ss: mu = fl(sum / m) carries those 11 u and the division's one, 12 u relative.  Each centred term fl((x - mu)^2) has two
# roundings of its own (2 u relative) and moves by 2 |x - mu| |delta mu| <= 2 |x - mu| 12 u mu to first order when mu does; the
# zeros' term (m - nnz) mu^2 has three roundings and moves by 2 mu |delta mu| a cell, which is the same expression with x = 0.
# The tree adds 11 u (+ 1 for the last add) again.  Together
#     |ss - exact| <= 15 u ss + 12 u * 2 mu sum_j |x_ij - mu|    (j over all m cells)
# which is 1.7e-15 (ss + 2 mu sum_j |x_ij - mu|).  That is below the 1e-13 the project holds its sums of this length to
# (tests/util_mp_project.py: SUM_BOUND, FACTOR_BOUND), so that constant stands:
SUM_BOUND = 1e-13          # |sum - exact| <= SUM_BOUND * sum|x|   (integers: exact, the sums stay far below 2^53)
SS_BOUND = 1e-13           # |ss - exact|  <= SS_BOUND * (ss + 2 mu sum_j |x_ij - mu|)


# ---- the reference, line by line ---------------------------------------------------------------------------------------------
def has_mode(g):
    """R/utils.R:329-339.  ``table(g)`` (:331) counts every distinct value of the row, zeros included, levels ascending;
    ``tb[names(tb)]`` (:333) removes nothing; TRUE iff some count is below the next level's (:336)."""
    _, tb = np.unique(np.asarray(g, dtype=np.float64), return_counts=True)          # :331
    n = len(tb)                                                                     # :334
    if n < 2:                                                                       # :335
        return False
    for k in range(n - 1):                                                          # :336
        if tb[k] < tb[k + 1]:
            return True
    return False                                                                    # :337


def calc_vmr(count, save_memory=False):
    """R/utils.R:197-218, with rowVars (:341-344) for the default path."""
    count = np.asarray(count, dtype=np.float64)
    gmean = count.mean(axis=1)                                                      # :199
    if not save_memory:
        var = ((count - gmean[:, None]) ** 2).sum(axis=1) / (count.shape[1] - 1)    # :343
    else:
        denom = count.shape[1]                                                      # :209
        var = np.empty(count.shape[0])
        for i in range(count.shape[0]):                                             # :210
            g = count[i] - gmean[i]                                                 # :211
            var[i] = (g * g).sum() / denom                                          # :212
    with np.errstate(divide="ignore", invalid="ignore"):
        return var / gmean                                                          # :217


def remove_zeros_idx(count):
    """Rows and columns ``remove_zeros`` keeps (R/utils.R:52, :94): those with a non-zero sum."""
    return np.flatnonzero(count.sum(axis=1) > 0), np.flatnonzero(count.sum(axis=0) > 0)


def filter_cells(count, umi_min=0, umi_max=np.inf):
    """R/utils.R:78-95 -> (rows kept, columns kept, message or None); rows / columns as indices into ``count``."""
    count = np.asarray(count, dtype=np.float64)
    umi = np.array([sum(float(v) for v in count[:, j] if v != 0) for j in range(count.shape[1])])    # :81, sequential
    selected = (umi_min <= umi) & (umi <= umi_max)                                  # :82
    msg = None
    if umi_min or umi_max < np.inf:                                                 # :90
        msg = f"{int(selected.sum())} cells out of {count.shape[1]} selected\n"     # :91
    cols = np.flatnonzero(selected)                                                 # :93
    r, c = remove_zeros_idx(count[:, cols])                                         # :94
    return r, cols[c], msg


def filter_genes(count, genes=None, markers=None, vmr_min=0, min_cells_expressed=0, max_cells_expressed=np.inf,
                 rescue_genes=False, save_memory=False):
    """R/utils.R:134-194 on a matrix WITHOUT empty genes handled the way the package documents: empty genes are dropped first.
    Returns a dict: rows kept (indices into ``count``), the logical vectors over the expressed genes, vmr, ncexpr, messages."""
    count = np.asarray(count, dtype=np.float64)
    nrow = count.shape[0]
    ncexpr = (count > 0).sum(axis=1)                                                # :139
    kept = np.flatnonzero(ncexpr > 0)
    count = count[kept]                                                             # :142
    ncexpr = ncexpr[kept]                                                           # :143
    ngenes = count.shape[0]                                                         # :144
    selected = np.zeros(ngenes, dtype=bool)                                         # :146
    marker_genes = None
    if markers is not None:                                                         # :148
        ncol = max(len(g) for g in genes)
        for k in range(ncol):                                                       # :150
            selected = selected | np.array([k < len(genes[i]) and genes[i][k] in markers for i in kept])   # :151-152
        marker_genes = selected.copy()                                              # :153
    vmr = calc_vmr(count, save_memory=save_memory)                                  # :156
    variable = (vmr_min < vmr) & (min_cells_expressed <= ncexpr) & (ncexpr <= max_cells_expressed)   # :159-161
    if rescue_genes and variable.sum() < ngenes:                                    # :162
        mode_genes = np.array([False if variable[i] else has_mode(count[i]) for i in range(ngenes)], dtype=bool)   # :166-169
        selected = selected | variable | mode_genes                                 # :173
    else:
        selected = selected | variable                                              # :176
        mode_genes = None                                                           # :177
    msg = ""
    if markers is not None and marker_genes.sum() > 0:                              # :180
        msg += f"{int(marker_genes.sum())} marker genes found\n"                    # :181
    if vmr_min > 0 or min_cells_expressed > 0 or max_cells_expressed < np.inf:      # :182
        msg += f"{int(variable.sum())} variable genes out of {nrow} \n"             # :183 (cat() puts a blank before '\n')
        if rescue_genes:
            msg += f"{int((selected & ~variable).sum())} additional genes rescued\n"    # :184-185
        msg += f"{int(selected.sum())} genes selected\n"                            # :186
    return {"rows": kept[selected], "selected_genes": selected, "variable_genes": variable, "mode_genes": mode_genes,
            "marker_genes": marker_genes, "vmr": vmr, "ncexpr": ncexpr, "messages": msg}


def normalize_count(count):
    """R/utils.R:318-327."""
    count = np.asarray(count, dtype=np.float64)
    umi = np.array([sum(float(v) for v in count[:, j] if v != 0) for j in range(count.shape[1])])    # :321, sequential
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (count.T / umi[:, None]).T                                            # :322
    med = np.median(umi)                                                            # :323
    out = out * med                                                                 # :324
    out[count == 0] = 0.0                                                           # (sparse: nothing is stored there)
    return out


# ---- one row in 50 digits ----------------------------------------------------------------------------------------------------
def mp_row(values, m):
    """(sum, ss, sum_abs, dev_abs) of a row with stored ``values`` among ``m`` cells, as floats of the 50-digit results:
    ss = sum over all m cells of (x - mu)^2, mu = sum / m; sum_abs = sum |x|; dev_abs = sum over all m cells of |x - mu|."""
    v = [mp.mpf(float(x)) for x in values]
    s = mp.fsum(v)
    mu = s / m
    zeros = m - len(v)
    ss = mp.fsum((x - mu) ** 2 for x in v) + zeros * mu ** 2
    dev = mp.fsum(abs(x - mu) for x in v) + zeros * abs(mu)
    return s, ss, mp.fsum(abs(x) for x in v), dev, mu


def row_errors(values, m, got_sum, got_ss):
    """(|sum - ref| / sum|x|, |ss - ref| / (ss_ref + 2 mu sum_j |x_ij - mu|)): the two figures the bounds above are set on;
    0 where the denominator is 0 and the result exact, inf where it is 0 and the result is not."""
    s, ss, sa, dev, mu = mp_row(values, m)
    es, ess = abs(mp.mpf(float(got_sum)) - s), abs(mp.mpf(float(got_ss)) - ss)
    ds, dss = sa, ss + 2 * abs(mu) * dev
    rs = float(es / ds) if ds > 0 else (0.0 if es == 0 else float("inf"))
    rss = float(ess / dss) if dss > 0 else (0.0 if ess == 0 else float("inf"))
    return rs, rss


# ---- cases -------------------------------------------------------------------------------------------------------------------
def row_from_table(table, m, rng):
    """A dense row of m cells holding ``table`` = {value: number of cells}, at seeded positions."""
    row = np.zeros(m)
    pos = rng.permutation(m)
    k = 0
    for v, c in table.items():
        row[pos[k:k + c]] = v
        k += c
    assert k <= m
    return row


def constructed_rows(B, m=300, seed=11):
    """The has_mode table of the issue: (dense rows [14][m], expected has_mode, tables).  B: the kernel's bin count."""
    tables = [
        ({1: 1}, False),
        ({1: 10, 2: 10}, False),                  # a tie
        ({1: 10, 2: 11}, True),
        ({1: 200}, True),                         # through the zeros: 100 < 200
        ({1: 150}, False),                        # 150 = 150
        ({3: 300}, False),                        # one level
        ({1: 100, 2: 200}, True),                 # no zeros
        ({1: 200, 2: 100}, False),
        ({5: 3, 9: 4}, True),
        ({5: 4, 9: 3}, False),                    # absent values are not levels
        ({B - 1: 2, 1: 1}, True),
        ({B: 2, 1: 1}, True),                     # decided by the host finisher
        ({B + 1: 2, 1: 1}, True),                 # decided by the host finisher
        ({2.5: 3, 1: 2}, True),                   # decided by the host finisher
    ]
    rng = np.random.default_rng(seed)
    X = np.stack([row_from_table(t, m, rng) for t, _ in tables])
    return X, np.array([e for _, e in tables], dtype=bool), [t for t, _ in tables]


def rows_for_host(X, bins):
    """Rows holding a stored value that is not an integer in [1, bins): the ones the kernel must leave to the host."""
    bad = (X != 0) & ~((X >= 1) & (X < bins) & (X == np.floor(X)))
    return bad.any(axis=1)


def length_rows(S, P, kind, seed=5):
    """One gene each of lengths 1, 2, S-1, S, S+1, P-1, P, P+1, 2P+1 among m = 2P+1 cells.  kind: 'small' counts 1..5,
    'large' counts 1e4..1e6 beside ones, 'frac' non-integer values."""
    m = 2 * P + 1
    lens = [1, 2, S - 1, S, S + 1, P - 1, P, P + 1, 2 * P + 1]
    rng = np.random.default_rng(seed)
    X = np.zeros((len(lens), m))
    for i, ln in enumerate(lens):
        pos = np.sort(rng.choice(m, size=ln, replace=False))
        if kind == "small":
            v = rng.integers(1, 6, size=ln).astype(np.float64)
        elif kind == "large":
            v = np.where(rng.random(ln) < 0.5, 1.0, np.floor(10.0 ** rng.uniform(4, 6, size=ln)))
        else:
            v = rng.gamma(0.7, 3.0, size=ln) + 1e-3
        X[i, pos] = v
    return X, lens


def many_genes(count, m=8, seed=9):
    """``count`` genes of one to three entries each (counts 1..4) among m cells."""
    rng = np.random.default_rng(seed)
    X = np.zeros((count, m))
    k = rng.integers(1, 4, size=count)
    for i in range(count):
        X[i, rng.choice(m, size=k[i], replace=False)] = rng.integers(1, 5, size=k[i])
    return X


def dense_stats(X):
    """nnz, sum, ss, has_mode of every row of a dense array, in numpy."""
    X = np.asarray(X, dtype=np.float64)
    mu = X.sum(axis=1) / X.shape[1]
    return ((X != 0).sum(axis=1), X.sum(axis=1), ((X - mu[:, None]) ** 2).sum(axis=1), np.array([has_mode(r) for r in X], dtype=bool))
