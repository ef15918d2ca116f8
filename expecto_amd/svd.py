"""Drop-in for the reference ``svd.py`` and ``svd_transform.py`` CLIs: the truncated SVD of the tf-idf
matrix of the chromatin-mark tracks, and the marks' coordinates in it (``tf_idf_reduced_100.npy``,
the file ``cluster_and_viz.py`` reads).

    python -m expecto_amd.svd <replicate_dir> --belugaFeatures features.tsv [ablation flags] \\
        [-o temp_svd] [--n_components 100] [--gene-batch 256]
    python -m expecto_amd.svd transform <replicate_dir> <temp_svd/svd_100.npz> --belugaFeatures features.tsv \\
        [ablation flags] [-o temp_svd_transform] [--gene-batch 256]

``<replicate_dir>`` holds one ``[S, marks]`` float32 ``.npy`` per gene (S = 200 in the reference).
Column ``g*S + s`` of the ``[kept marks, genes*S]`` track matrix is row ``s`` of file ``g``.  With
``x`` the kept marks' tracks, in float64 on the float32 inputs (svd.py:76-81):

    r_i = sum_n x[n,i]     idf_n = log(m / (1 + sum_i x[n,i]))     A[i,n] = x[n,i] / r_i * idf_n

The reference runs sklearn's randomized ``TruncatedSVD(100)`` on ``A`` in float32, after building
``A`` and two temporaries of its size on the host.  There are at most 2002 marks, so here the exact
route is taken: the float64 Gram matrix ``G = A A^T`` is accumulated on the device over chunks of
files (``expecto_tfidf_stats``, ``expecto_tfidf_gram``), ``numpy.linalg.eigh`` solves the ``m x m``
eigenproblem on the host, and a second pass over the files projects them into ``components_``
(``expecto_tfidf_project``).  The result is deterministic and exact to float64 rounding; the
reference's trailing components are approximate.  Signs follow sklearn >= 1.5
(``svd_flip(u_based_decision=False)``): the largest-magnitude entry of each ``components_`` row is
positive, the first one on ties.

Differences from the reference, on purpose:
* files are taken in sorted order (the reference uses ``glob`` order, which is arbitrary); the
  columns of ``components_`` follow that order, ``x_reduced`` does not depend on it beyond rounding;
* it works with no ablation flag (the reference calls ``.values`` on the ndarray ``get_keep_mask``
  returns then, and crashes);
* the model is ``svd_<k>.npz`` (``components_``, ``singular_values_``, ``explained_variance_``,
  ``explained_variance_ratio_``, ``x_reduced``, ``files``, ``keep_idx``, ``rows_per_file``); the fit
  also writes ``tf_idf_reduced_<k>.npy`` for the fitted directory.  ``transform`` accepts a sklearn
  ``.joblib`` dump where joblib and scikit-learn are installed, together with ``--file-order``: the
  files' basenames in the order of the dump's columns (the fitting run's ``glob`` order, which the
  dump does not record); without it such a dump is refused.
"""
from __future__ import annotations

import argparse
import glob
import os
import sys

import numpy as np

N_COMPONENTS = 100      # svd.py:84
GENE_BATCH = 256
# A kept eigenvalue below lambda_1 * m * 2^-52 * 2^20 is refused: the Gram route's relative error in
# lambda_c is about m * 2^-52 * lambda_1 / lambda_c, which this keeps below ~1e-6.
EIG_FLOOR = 2.0 ** -52 * 2.0 ** 20


def _add_common(parser):
    parser.add_argument('replicate_expecto_features_dir')


def _add_flags(parser, out_default):
    parser.add_argument('--belugaFeatures', action="store", dest="belugaFeatures",
                        help="tsv file denoting Beluga features")
    parser.add_argument('--no_tf_features', action='store_true', dest='no_tf_features', default=False,
                        help='leave out TF marks for training')
    parser.add_argument('--no_dnase_features', action='store_true', dest='no_dnase_features', default=False,
                        help='leave out DNase marks for training')
    parser.add_argument('--no_histone_features', action='store_true', dest='no_histone_features', default=False,
                        help='leave out histone marks for training')
    parser.add_argument('--intersect_with_lambert', action='store_true', dest='intersect_with_lambert', default=False,
                        help='intersect with Lambert2018_TFs_v_1.01_curatedTFs.csv')
    parser.add_argument('--no_pol2', action='store_true', dest='no_pol2', default=False, help='take out Pol2*')
    parser.add_argument('-o', dest="out_dir", type=str, default=out_default, help='Output directory')
    parser.add_argument('--gene-batch', dest="gene_batch", type=int, default=GENE_BATCH,
                        help='files per device chunk')


def build_parser():
    """The arguments of svd.py:20-41, plus --n_components and --gene-batch."""
    parser = argparse.ArgumentParser(prog="python -m expecto_amd.svd", description='Compute SVD')
    _add_common(parser)
    _add_flags(parser, 'temp_svd')
    parser.add_argument('--n_components', type=int, default=N_COMPONENTS)
    return parser


def build_transform_parser():
    """The arguments of svd_transform.py:20-42, plus --gene-batch."""
    parser = argparse.ArgumentParser(prog="python -m expecto_amd.svd transform",
                                     description='Compute SVD transform of training data')
    _add_common(parser)
    parser.add_argument('svd_joblib', help="svd_<k>.npz of a fit (or a sklearn TruncatedSVD joblib dump)")
    _add_flags(parser, 'temp_svd_transform')
    parser.add_argument('--file-order', dest="file_order", type=str, default=None,
                        help="with a sklearn joblib dump: text file of the gene files' basenames, one per line, in "
                             "the order of the dump's components_ columns (the fitting run's glob order)")
    return parser


# ---- inputs ----------------------------------------------------------------------------------

class _Files:
    """The per-gene inputs: paths (taken in sorted order, or in the order of the basenames ``order``
    where that lists exactly these files) or [S, marks] arrays (in the given order)."""

    def __init__(self, files, order=None):
        files = list(files)
        if not files:
            raise ValueError("svd: no input files")
        self.paths = all(isinstance(f, (str, os.PathLike)) for f in files)
        if self.paths:
            files = sorted(os.fspath(f) for f in files)
            self.names = [os.path.basename(f) for f in files]
            if order is not None and sorted(str(s) for s in order) == sorted(self.names) and \
                    len(set(self.names)) == len(self.names):
                at = {name: f for name, f in zip(self.names, files)}
                self.names = [str(s) for s in order]
                files = [at[name] for name in self.names]
        else:
            if any(isinstance(f, (str, os.PathLike)) for f in files):
                raise ValueError("svd: pass either paths or arrays, not both")
            self.names = [f"<array {i}>" for i in range(len(files))]
        self.items = files
        for g in range(len(files)):     # every shape is checked before the device is touched
            shape = self._load(g, mmap_mode="r").shape
            if len(shape) != 2:
                raise ValueError(f"svd: {self.names[g]} has shape {shape}, expected [rows, marks]")
            if g == 0:
                self.rows, self.marks = shape
            elif shape != (self.rows, self.marks):
                raise ValueError(f"svd: {self.names[g]} has shape {shape}, {self.names[0]} has "
                                 f"{(self.rows, self.marks)}")

    def _load(self, g, mmap_mode=None):
        return np.load(self.items[g], mmap_mode=mmap_mode) if self.paths else np.asarray(self.items[g])

    def __len__(self):
        return len(self.items)

    @property
    def columns(self):
        return len(self.items) * self.rows

    def chunks(self, gene_batch):
        """(first column, float32 [n, marks] host array) per chunk of ``gene_batch`` files."""
        if gene_batch < 1:
            raise ValueError("svd: gene_batch must be at least 1")
        for g0 in range(0, len(self.items), gene_batch):
            g1 = min(g0 + gene_batch, len(self.items))
            block = np.empty((g1 - g0, self.rows, self.marks), np.float32)
            for g in range(g0, g1):
                block[g - g0] = self._load(g)
            yield g0 * self.rows, block.reshape(-1, self.marks)


def _check_keep(keep_idx, marks):
    keep = np.asarray(keep_idx)
    if keep.dtype == bool:
        keep = np.nonzero(keep)[0]
    keep = keep.astype(np.int64).ravel()
    if keep.size and (keep.min() < 0 or keep.max() >= marks):
        raise ValueError(f"svd: keep_idx entries must lie in [0, {marks})")
    if np.unique(keep).size != keep.size:
        raise ValueError("svd: keep_idx entries must be distinct")
    return keep


class _Device:
    """The device side of both passes: the library, the kept marks and the buffers a chunk needs."""

    def __init__(self, keep, device):
        from . import _lib
        torch = _lib.require_gpu("svd")
        self.torch, self._lib, self.lib = torch, _lib, _lib.load()
        self.dev = _lib.device_of(device)
        self.m = int(keep.size)
        with torch.cuda.device(self.dev):
            self.keep = torch.from_numpy(keep.astype(np.int32)).to(self.dev)
            self.rowsum = torch.zeros(self.m, dtype=torch.float64, device=self.dev)
        self.ws = None

    def call(self, name, *args):
        with self.torch.cuda.device(self.dev):
            self._lib.call(name, *args)

    def upload(self, host):
        return self._lib.upload(host, self.dev)

    def workspace(self, nbytes):
        if self.ws is None or self.ws.numel() * 8 < nbytes:
            self.ws = self._lib.workspace(nbytes, self.dev)
        return self.ws

    def stats(self, D, idf):
        n, ld = D.shape
        self.call("expecto_tfidf_stats", D.data_ptr(), n, ld, self.keep.data_ptr(), self.m, idf.data_ptr(),
                  self.rowsum.data_ptr())

    def checked_rowsum(self, idf):
        """The row sums on the host, after the refusals that the statistics decide."""
        r = self.rowsum.cpu().numpy()
        if not np.isfinite(r).all():
            raise ValueError("svd: the tracks contain NaN or infinity")
        if not bool(self.torch.isfinite(idf).all()):
            bad = int((~self.torch.isfinite(idf)).sum())
            raise ValueError(f"svd: {bad} column(s) hold NaN or infinity, or have 1 + column sum <= 0 "
                             "(the inverse document frequency log(m / (1 + sum)) is not finite)")
        if (r <= 0).any():
            raise ValueError(f"svd: {int((r <= 0).sum())} kept mark(s) have a row sum <= 0 (first: kept mark "
                             f"{int(np.nonzero(r <= 0)[0][0])}); the term frequency x / sum is undefined")
        return r


def _pass_stats(files, devs, gene_batch, with_gram):
    """Pass 1: idf of every column, the row sums and (``with_gram``) H = sum_n t t^T, over the chunks."""
    torch = devs.torch
    N, m = files.columns, devs.m
    with torch.cuda.device(devs.dev):
        idf = torch.empty(N, dtype=torch.float64, device=devs.dev)
        H = torch.zeros((m, m), dtype=torch.float64, device=devs.dev) if with_gram else None
    for n0, host in files.chunks(gene_batch):
        D = devs.upload(host)
        n = D.shape[0]
        devs.stats(D, idf[n0:n0 + n])
        if with_gram:
            nbytes = int(devs.lib.expecto_tfidf_gram_workspace(m, n))
            ws = devs.workspace(nbytes)
            devs.call("expecto_tfidf_gram", D.data_ptr(), n, D.shape[1], devs.keep.data_ptr(), m,
                      idf[n0:n0 + n].data_ptr(), H.data_ptr(), ws.data_ptr(), nbytes)
    return idf, H


def sign_flip(components):
    """Signs (+1 / -1, float64 [k]) that make the largest-magnitude entry of each row positive, the
    first such entry on ties: sklearn >= 1.5 ``svd_flip(u, v, u_based_decision=False)``."""
    components = np.asarray(components)
    at = np.argmax(np.abs(components), axis=1)
    s = np.sign(components[np.arange(components.shape[0]), at]).astype(np.float64)
    s[s == 0] = 1.0
    return s


def eig_top(G, k):
    """The k largest eigenpairs of the symmetric G, descending: (lambda [k], Q [m, k]).  ValueError if
    a kept eigenvalue lies below the floor under which the Gram route loses its accuracy."""
    m = G.shape[0]
    lam, Q = np.linalg.eigh(G)
    lam, Q = lam[::-1][:k], Q[:, ::-1][:, :k]
    floor = lam[0] * m * EIG_FLOOR
    low = int((lam < floor).sum())
    if low:
        raise ValueError(f"svd: {low} of the {k} requested components have an eigenvalue below "
                         f"{floor:.3e} = lambda_1 * m * 2^-32, where the float64 Gram matrix no longer resolves them; "
                         f"ask for at most {k - low} components")
    return lam, np.ascontiguousarray(Q)


def full_variance(G):
    """sum of the column variances of A for G = A A^T: trace(G)/m - sum(G)/m^2."""
    m = G.shape[0]
    return float(np.trace(G) / m - G.sum() / (m * m))


def fit(files, keep_idx, n_components=N_COMPONENTS, gene_batch=GENE_BATCH, device=None) -> dict:
    """Truncated SVD of the tf-idf matrix of ``files`` (paths, taken in sorted order, or ``[S, marks]``
    arrays) restricted to the marks ``keep_idx``.  Returns a dict: ``components_`` (float32 [k, N]),
    ``singular_values_``, ``explained_variance_``, ``explained_variance_ratio_`` (float64 [k]),
    ``x_reduced`` (float64 [m, k]: the fitted marks' coordinates, ``svd.transform`` of the fitted
    data), ``files`` (basenames in column order), ``keep_idx`` and ``rows_per_file``.

    ValueError: a NaN or infinity in the tracks, a kept mark whose row sum is <= 0, a column with
    1 + sum <= 0, more components than marks or columns, or components the Gram route cannot resolve."""
    files = _Files(files)
    keep = _check_keep(keep_idx, files.marks)
    m, N, k = int(keep.size), files.columns, int(n_components)
    if k < 1:
        raise ValueError("svd: n_components must be at least 1")
    if k > m or k > N:
        raise ValueError(f"svd: n_components = {k} exceeds the {m} kept marks or the {N} columns")
    devs = _Device(keep, device)
    torch = devs.torch

    idf, H = _pass_stats(files, devs, gene_batch, True)
    r = devs.checked_rowsum(idf)
    G = H.cpu().numpy() / np.outer(r, r)
    del H
    lam, Q = eig_top(G, k)
    sigma = np.sqrt(lam)

    with torch.cuda.device(devs.dev):
        P = devs.upload(np.ascontiguousarray((Q / (sigma[None, :] * r[:, None])).T))       # [k, m]
        comps = torch.empty((k, N), dtype=torch.float32, device=devs.dev)
    for n0, host in files.chunks(gene_batch):
        D = devs.upload(host)
        n = D.shape[0]
        devs.call("expecto_tfidf_project", D.data_ptr(), n, D.shape[1], devs.keep.data_ptr(), m,
                  idf[n0:n0 + n].data_ptr(), P.data_ptr(), k, comps.data_ptr() + 4 * n0, N)
    components = comps.cpu().numpy()
    del comps
    signs = sign_flip(components)
    components *= signs[:, None].astype(np.float32)
    x_reduced = Q * (sigma * signs)[None, :]
    ev = np.var(x_reduced, axis=0)
    return {"components_": components, "singular_values_": sigma, "explained_variance_": ev,
            "explained_variance_ratio_": ev / full_variance(G), "x_reduced": x_reduced,
            "files": list(files.names), "keep_idx": keep, "rows_per_file": int(files.rows)}


def transform(model, files, gene_batch=GENE_BATCH, device=None) -> np.ndarray:
    """``svd.transform(tf_idf)`` of the track matrix of ``files``: float64 [m, k].  ``files`` must be the
    model's: the same basenames, the same count and rows per file, since ``components_`` has one
    column per track column.  Paths are read in the order of the model's ``files`` (sorted order for
    a model of :func:`fit`; the recorded ``glob`` order for a reference dump, see :func:`load_model`)."""
    files = _Files(files, order=model.get("files"))
    components = np.ascontiguousarray(model["components_"], np.float32)
    k, N = components.shape
    keep = _check_keep(model["keep_idx"], files.marks)
    rows = model.get("rows_per_file")
    if rows is not None and int(rows) != files.rows:
        raise ValueError(f"svd transform: the files have {files.rows} rows each, the model was fitted on "
                         f"{int(rows)} rows per file")
    names = model.get("files")
    if names is not None:
        names = [str(s) for s in names]
        if len(names) != len(files):
            raise ValueError(f"svd transform: {len(files)} files given, the model was fitted on {len(names)}")
        if files.paths and names != files.names:
            k_bad = next(i for i, (a, b) in enumerate(zip(names, files.names)) if a != b)
            raise ValueError(f"svd transform: file {k_bad} is {files.names[k_bad]}, the model was fitted on "
                             f"{names[k_bad]} there (basenames differ)")
    if files.columns != N:
        raise ValueError(f"svd transform: the files hold {files.columns} columns ({len(files)} files of {files.rows} "
                         f"rows), the model's components have {N}")
    devs = _Device(keep, device)
    torch = devs.torch
    m = devs.m
    with torch.cuda.device(devs.dev):
        X = torch.zeros((m, k), dtype=torch.float64, device=devs.dev)
        idf = torch.empty(N, dtype=torch.float64, device=devs.dev)
    for n0, host in files.chunks(gene_batch):
        D = devs.upload(host)
        n = D.shape[0]
        devs.stats(D, idf[n0:n0 + n])
        V = devs.upload(np.ascontiguousarray(components[:, n0:n0 + n]))
        nbytes = int(devs.lib.expecto_tfidf_transform_workspace(m, k, n))
        ws = devs.workspace(nbytes)
        devs.call("expecto_tfidf_transform", D.data_ptr(), n, D.shape[1], devs.keep.data_ptr(), m,
                  idf[n0:n0 + n].data_ptr(), V.data_ptr(), n, k, X.data_ptr(), ws.data_ptr(), nbytes)
    r = devs.checked_rowsum(idf)
    return X.cpu().numpy() / r[:, None]


# ---- model files -----------------------------------------------------------------------------

MODEL_KEYS = ("components_", "singular_values_", "explained_variance_", "explained_variance_ratio_", "x_reduced",
              "files", "keep_idx", "rows_per_file")


def save_model(path: str, model: dict) -> None:
    np.savez(path, **{key: (np.asarray(model[key], dtype=str) if key == "files" else np.asarray(model[key]))
                      for key in MODEL_KEYS})


def load_model(path: str, keep_idx=None, file_order=None, rows_per_file=None) -> dict:
    """The dict of :func:`fit` from a ``svd_<k>.npz``; or, from a sklearn ``TruncatedSVD`` joblib dump,
    its ``components_`` with ``keep_idx`` and ``file_order``.  Such a dump records neither the marks
    nor the files, and the reference's columns follow its ``glob`` order, which is arbitrary: without
    the basenames in that order (``file_order``) the columns cannot be paired with files, so the
    dump is refused rather than transformed into wrong numbers."""
    if path.endswith(".npz"):
        with np.load(path) as z:
            model = {key: z[key] for key in MODEL_KEYS}
        model["files"] = [str(s) for s in model["files"]]
        model["rows_per_file"] = int(model["rows_per_file"])
        return model
    try:
        import joblib
        import sklearn  # noqa: F401  -- the dump unpickles into its classes
    except ImportError as e:
        raise RuntimeError(f"{path}: reading a sklearn joblib dump needs joblib and scikit-learn ({e}); pass the "
                           "svd_<k>.npz this program writes instead") from e
    if keep_idx is None:
        raise ValueError(f"{path}: a sklearn dump does not record the kept marks; pass keep_idx")
    if file_order is None:
        raise ValueError(f"{path}: a sklearn dump does not record the order of the files its components_ columns "
                         "follow (the reference takes glob order, which is arbitrary); pass the basenames in that "
                         "order (--file-order FILE, one name per line)")
    svd = joblib.load(path)
    return {"components_": np.asarray(svd.components_, np.float32), "keep_idx": np.asarray(keep_idx),
            "singular_values_": getattr(svd, "singular_values_", None), "files": [str(s) for s in file_order],
            "rows_per_file": rows_per_file}


# ---- CLI -------------------------------------------------------------------------------------

def _inputs(args):
    """svd.py:49-74: the directory's files and the kept marks; prints the reference's two lines."""
    from . import predict

    npy_files = sorted(glob.glob(f'{args.replicate_expecto_features_dir}/*.npy'))
    if not npy_files:
        raise ValueError(f"no .npy files in {args.replicate_expecto_features_dir}")
    beluga_features_df = predict.read_features_table(args.belugaFeatures)
    keep_mask = predict.get_keep_mask(beluga_features_df, *predict.mask_arguments(args))
    keep_indices = np.nonzero(np.asarray(keep_mask))[0]
    rows, marks = np.load(npy_files[0], mmap_mode="r").shape
    if marks != beluga_features_df.shape[0]:
        raise ValueError(f"{npy_files[0]} has {marks} marks, --belugaFeatures lists {beluga_features_df.shape[0]}")
    print(f'Tracks shape: {(len(keep_indices), len(npy_files) * rows)}')
    return npy_files, keep_indices


def run_fit(args):
    os.makedirs(args.out_dir, exist_ok=True)
    npy_files, keep_indices = _inputs(args)
    model = fit(npy_files, keep_indices, n_components=args.n_components, gene_batch=args.gene_batch)
    k = args.n_components
    save_model(f'{args.out_dir}/svd_{k}.npz', model)
    np.save(f'{args.out_dir}/tf_idf_reduced_{k}', model["x_reduced"].astype(np.float32))
    return model


def run_transform(args):
    os.makedirs(args.out_dir, exist_ok=True)
    npy_files, keep_indices = _inputs(args)
    order = None
    if args.file_order is not None:
        with open(args.file_order) as f:
            order = f.read().split()
    model = load_model(args.svd_joblib, keep_idx=keep_indices, file_order=order)
    if not np.array_equal(np.asarray(model["keep_idx"]), keep_indices):
        raise ValueError(f"{args.svd_joblib} was fitted on {len(model['keep_idx'])} kept marks that differ from the "
                         f"{len(keep_indices)} the ablation flags of this run keep")
    X = transform(model, npy_files, gene_batch=args.gene_batch)
    np.save(f'{args.out_dir}/tf_idf_reduced_{X.shape[1]}', X.astype(np.float32))
    return X


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv and argv[0] == "transform":
        return run_transform(build_transform_parser().parse_args(argv[1:]))
    return run_fit(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
