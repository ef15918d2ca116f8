"""numpy restatements of the attribution step (tests/test_contrib_host.py, tests/test_gpu_contrib.py).

* ``reference_order`` -- ``interpret_model`` and ``interpret_model_with_clusters[_rsat]``
  (predict_by_cluster.py:73-109, predict_by_cluster_rsat.py:105-144) with the reference's own
  numpy / pandas calls, on the ``[n, 10*nk]`` ref / alt feature matrices it builds.
* ``device_order`` -- the order ``expecto_variant_contrib`` documents (include/expecto_hip.h):
  contributions summed over the decay rows left to right, totals and cluster sums by ``wave_sum``.
* ``bounds`` -- how far the two may differ.  Both sum the same rounded products ``w * D[k]`` in
  another order; a float64 sum of N terms in any order is within ``(N-1) * 2^-53 * sum|terms|``
  of the exact sum, so two orders are within ``N * 2^-52 * sum|terms|`` of each other:
  ``|contrib_d - contrib_r| <= 10 * 2^-52 * sum_k |w*D[k]|``, totals and cluster sums the same
  with the member count and ``sum |contrib|``.  A proportion ``c / t`` moves by at most
  ``(|dc| + |c/t| * |dt|) / |t|`` to first order; the second-order term is below ``dt / |t|``
  of that (< 1e-6 where ``|t| >= 1e-3 * sum|contrib|``, covered by the factor 1.001), and the two
  divisions round once each (``2^-52 * |c/t|`` together).
"""
import numpy as np
import pandas as pd

EPS = 2.0 ** -52


def wave_sum(x):
    """S(x) over the last axis in the kernel's order: 64 strided left-to-right lane sums (-0.0
    where a lane has no term), folded 32, 16, 8, 4, 2, 1; +0.0 for no terms."""
    x = np.asarray(x, np.float64)
    c = x.shape[-1]
    if c == 0:
        return np.zeros(x.shape[:-1])
    pad = np.full(x.shape[:-1] + ((-c) % 64,), -0.0)
    rows = np.concatenate([x, pad], -1).reshape(x.shape[:-1] + (-1, 64))
    p = rows[..., 0, :].copy()
    for i in range(1, rows.shape[-2]):
        p = p + rows[..., i, :]
    s = 32
    while s:
        p = p[..., :s] + p[..., s:2 * s]
        s //= 2
    return p[..., 0]


def device_order(ref_feat, alt_feat, nfeat, keep, w, clusters=None):
    """ref_feat, alt_feat [n, 10*nfeat] f64 (the variant reduction's outputs); keep [nk];
    w [M, 10*nk]; clusters: lists of indices into keep.  Returns a dict of the five outputs
    ([M, n, ...]; clu and clu_prop None without clusters)."""
    keep = np.asarray(keep)
    n, nk = ref_feat.shape[0], len(keep)
    D = alt_feat.reshape(n, 10, nfeat)[:, :, keep] - ref_feat.reshape(n, 10, nfeat)[:, :, keep]
    W = np.asarray(w, np.float64).reshape(-1, 10, nk)
    c = W[:, None, 0, :] * D[None, :, 0, :]
    for k in range(1, 10):
        c = c + W[:, None, k, :] * D[None, :, k, :]
    out = {"contrib": c, "total": wave_sum(c), "clu": None, "clu_prop": None}
    with np.errstate(all="ignore"):
        out["prop"] = c / out["total"][..., None]
        if clusters is not None and len(clusters):
            clu = np.stack([wave_sum(c[..., np.asarray(m, np.int64)]) for m in clusters], -1)
            out["clu"], out["clu_prop"] = clu, clu / wave_sum(clu)[..., None]
    return out


def _preds_per_feature(weights, ref_features, alt_features):
    preds_per_feature = (weights * (alt_features - ref_features))          # predict_by_cluster_rsat.py:110-113
    return preds_per_feature.ravel() \
        .reshape(preds_per_feature.shape[0], 10, preds_per_feature.shape[1] // 10) \
        .transpose(0, 2, 1)


def reference_order(weights, ref_features, alt_features, clusters=None):
    """One model's weights [10*nk] on features [n, 10*nk].  clusters: a list of cluster-id lists
    per mark (rsat mode), a pandas Series of one label per mark (``--feature_clusters_df`` mode), or
    None.  Returns contrib, total, prop [n, nk] and, with clusters, clu, clu_prop [n, n_clu] and
    ``columns`` (the cluster ids in the reference's column order)."""
    weights = np.asarray(weights, np.float64)
    ppf = _preds_per_feature(weights, ref_features, alt_features)         # (n_snps, n_marks, 10)
    contrib = ppf.sum(axis=-1)                                            # :115
    total = contrib.sum(axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        out = {"contrib": contrib, "total": total[:, 0], "prop": contrib / total}        # :116
    if clusters is None:
        return out
    preds_per_feature_df = pd.DataFrame(ppf.reshape(ppf.shape[0], -1).T)  # (n_input_features, n_snps)  :132
    if isinstance(clusters, pd.Series):                                   # predict_by_cluster.py:102-107
        cluster_labels = np.repeat(clusters.values, 10)
        assert cluster_labels.shape[0] == preds_per_feature_df.shape[0]
        preds_per_feature_df['cluster'] = cluster_labels
        grouped = preds_per_feature_df.groupby('cluster').sum()
        cluster_contribs, columns = grouped.values.T, list(range(grouped.shape[0]))
    else:                                                                 # predict_by_cluster_rsat.py:135-143
        acc = {}
        for fi in range(preds_per_feature_df.shape[0]):
            feature_preds = preds_per_feature_df.iloc[fi]
            for cluster_id in clusters[fi // 10]:
                acc[cluster_id] = acc.get(cluster_id, 0) + feature_preds
        frame = pd.DataFrame(acc)
        cluster_contribs, columns = frame.values, list(frame.columns)
    with np.errstate(all="ignore"):
        out.update(clu=cluster_contribs, columns=columns,
                   clu_prop=cluster_contribs / cluster_contribs.sum(axis=-1, keepdims=True))
    return out


def bounds(weights, ref_features, alt_features, ref, members=None):
    """Allowed |device - reference| per output of one model (module docstring), from the reference's
    own values ``ref`` (``reference_order``).  members: the marks of every cluster column, in the
    order of ``ref['columns']``."""
    ppf = np.abs(_preds_per_feature(np.asarray(weights, np.float64), ref_features, alt_features))
    nk = ppf.shape[1]
    b = {"contrib": 10 * EPS * ppf.sum(-1)}
    sum_c = np.abs(ref["contrib"]).sum(-1)
    b["total"] = nk * EPS * sum_c
    t = np.abs(ref["total"])[:, None]
    b["prop"] = 1.001 * (b["contrib"] + np.abs(ref["prop"]) * b["total"][:, None]) / t + EPS * np.abs(ref["prop"])
    b["prop_rows"] = np.abs(ref["total"]) >= 1e-3 * sum_c
    if members is not None:
        b["clu"] = np.stack([len(m) * EPS * np.abs(ref["contrib"][:, list(m)]).sum(-1) for m in members], -1)
        sum_u = np.abs(ref["clu"]).sum(-1)
        den = np.abs(ref["clu"].sum(-1))[:, None]
        b_den = b["clu"].sum(-1) + len(members) * EPS * sum_u
        b["clu_prop"] = 1.001 * (b["clu"] + np.abs(ref["clu_prop"]) * b_den[:, None]) / den + \
            EPS * np.abs(ref["clu_prop"])
        b["clu_rows"] = den[:, 0] >= 1e-3 * sum_u
    return b


def golden_inputs(golden_dir):
    """The inputs of the golden run (tests/golden/make_golden_contribs.py) as the reference's
    interpretation step sees them: kept marks, HGNC table, dump weights, [7, 10*40] ref / alt
    features (the matrices the reference predict.py built, predict_features.npz), clusters."""
    import os

    from expecto_amd import predict
    from expecto_amd.xgblinear import GBLinear
    pbc = os.path.join(golden_dir, "predict_by_cluster")
    cwd = os.getcwd()
    os.chdir(pbc)                       # ./resources/*.csv, as the reference reads them
    try:
        df = predict.read_features_table(os.path.join(golden_dir, "predict_sed", "deepsea_beluga_2002_features.tsv"))
        keep_mask, hgnc_df = predict.get_keep_mask(df, False, False, False, True, False, return_hgnc_df=True)
    finally:
        os.chdir(cwd)
    keep = np.nonzero(keep_mask)[0]
    feats = np.load(os.path.join(golden_dir, "predict_features.npz"))
    cols = (np.arange(10)[:, None] * 2002 + keep[None, :]).reshape(-1)
    weights = GBLinear.load(os.path.join(pbc, "model.save")).dump_weights()
    tab = pd.read_csv(os.path.join(pbc, "clusters_motif_names.tab"), sep="\t", header=None)
    assay_clusters, not_found = rsat_assay_clusters(tab, hgnc_df[keep_mask]["Assay"])
    return dict(keep=keep, features=df, hgnc=hgnc_df[keep_mask], weights=weights, ref=feats["ref"][:, cols],
                alt=feats["alt"][:, cols], assay_clusters=assay_clusters, not_found=not_found)


def rsat_assay_clusters(tab_df, assays):
    """predict_by_cluster_rsat.py:78-102: per assay the 1-based ids of the rsat clusters whose
    upper-cased, ``_``-stripped motif names hold it, else [-1]; and the set of assays not found."""
    sets = tab_df[1].str.upper().str.split(',').apply(lambda ms: [m.split("_")[0] for m in ms]).apply(set)
    assay_clusters, not_found = [], set()
    for assay in assays:
        ids = [i + 1 for i, s in enumerate(sets.values) if assay in s]
        if not ids:
            ids = [-1]
            not_found.add(assay)
        assay_clusters.append(ids)
    return assay_clusters, not_found
