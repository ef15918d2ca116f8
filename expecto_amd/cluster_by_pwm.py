"""Drop-in for the reference ``cluster_by_pwm.py``, and the step that followed it outside the reference:
which TF motifs stand for the Beluga TF marks, and which of them are the same motif?

    python -m expecto_amd.cluster_by_pwm --belugaFeatures features.tsv --jaspar_motif_db JASPAR_DIR \\
        --hocomoco_jaspar_motif_file HOCOMOCO.jaspar [--cisbp2_meme_file X] [--no_cluster] \\
        [--cor 0.6 --ncor 0.4 --min_w 5 --pseudo 1.0] [-o temp_cluster_by_pwm]
    python -m expecto_amd.cluster_by_pwm --motif_file M.jaspar|M.meme [...] -o out_dir

Stage 1, on the host (``cluster_by_pwm.py:31-102``, the same arguments; ``--cisbp2_meme_file`` is accepted
and ignored, as its use is commented out there).  The marks are the TF marks whose HGNC name is in
Lambert's list, without Pol2 (``predict.get_keep_mask`` with the flags the reference hard-codes; it reads
``./resources/*.csv``).  A JASPAR motif, one per ``*.jaspar`` file, is kept when its upper-cased name is
such a mark's assay (``::`` heterodimers are skipped); a HOCOMOCO motif when its name up to the first
``_`` is.  ``cluster_motifs.jaspar`` holds the kept motifs.  The reference writes that file with
``Bio.motifs.write``; Biopython is not available to this project, so byte equality with it has not been
checked: the contract is that :func:`read_jaspar` reads the file back to the same IDs, names and counts
(to the two decimals of ``%6.2f``).  The ``*.jaspar`` files are read in sorted order (the reference
takes ``glob``'s).  ``--motif_file`` (JASPAR, or MEME through ``query_fimo_for_predictions.read_meme``
with counts = frequencies x nsites) skips the selection.

Stage 2, on the device, on by default (``--no_cluster`` stops after stage 1).  The reference hands
``cluster_motifs.jaspar`` to RSAT *matrix-clustering*, whose ``clusters_motif_names.tab`` is what
``predict_by_cluster --rsat_clusters_tab`` and ``cluster_analysis_with_fimo --rsat_clusters_file`` read.
Here that file comes from this module.  The arithmetic follows RSAT's published definitions of cor, Ncor
and average linkage, with matrix-clustering's documented default thresholds; no RSAT output was
available, so agreement with RSAT is by definition only and is unmeasured.

* frequencies ``f[j][b] = (c[j][b] + pseudo/4) / (((cA + cC) + cG) + cT + pseudo)``, float64, alphabet
  order; centred ``a = f - 0.25`` (the mean over whole columns is 0.25);
* per pair (A, B), strands D (B) and R (``B_rc[j][b] = B[wB-1-j][3-b]``), offsets ``o`` (A's column under
  B's column 0) from ``-(wB - need)`` to ``wA - need``, ``need = min(min_w, wA, wB)``: ``cor`` is the
  Pearson correlation of the centred overlap, ``Ncor = cor * w / (wA + wB - w)``; the best alignment has
  the largest Ncor, ties to D, then to the smaller ``o`` (``expecto_pwm_compare``, include/expecto_hip.h);
* ``dist = max(0, 1 - Ncor)``, scipy's average linkage of it (``expecto_average_linkage``, host);
* a merge holds when both sides hold and the mean cor and mean Ncor over its cross pairs reach ``--cor``
  and ``--ncor``; the clusters are the maximal merges that hold (``expecto_linkage_threshold_cut``, host).

Writes ``cluster_motifs.jaspar``, ``clusters_motif_names.tab`` (``cluster_k<TAB>name,name,...``, no header,
names in input order), ``pairwise_compa.tsv`` (``id1 id2 cor Ncor strand offset w``) and ``tree.npz``
(``children``, ``distances``, ``sizes``, ``mean_cor``, ``mean_ncor``).  RSAT's consensus and logo trees,
its other linkage methods and its plots are left out.
"""
from __future__ import annotations

import argparse
import glob
import os
import re
import sys
from typing import NamedTuple

import numpy as np

MAX_M, MAX_W = 4096, 64                      # include/expecto_hip.h
ALPHABET = "ACGT"


class Motif(NamedTuple):
    id: str
    name: str
    counts: np.ndarray         # float64 [w, 4], alphabet order


class Comparison(NamedTuple):
    """Best alignment of every pair (i < j), scipy's condensed order."""
    cor: np.ndarray            # float64
    ncor: np.ndarray           # float64
    dist: np.ndarray           # float64: max(0, 1 - Ncor)
    offset: np.ndarray         # int32: column of motif i under column 0 of motif j
    strand: np.ndarray         # int32: 0 D, 1 R
    width: np.ndarray          # int32: columns of the overlap


class Tree(NamedTuple):
    children: np.ndarray       # int32 [n-1, 2]
    distances: np.ndarray      # float64 [n-1]
    sizes: np.ndarray          # int32 [n-1]


class Cut(NamedTuple):
    labels: np.ndarray         # int32 [n], 1-based, by ascending smallest member
    mean_cor: np.ndarray       # float64 [n-1]
    mean_ncor: np.ndarray      # float64 [n-1]


class Clustering(NamedTuple):
    comparison: Comparison
    tree: Tree
    cut: Cut

    @property
    def labels(self):
        return self.cut.labels


# ---- JASPAR text -------------------------------------------------------------------------------

_HEADER = re.compile(r"^>\s*(\S+)(?:\s+(\S+))?")
_ROW = re.compile(r"^\s*([ACGTacgt])\s*\[?\s*([^\]]*?)\s*\]?\s*$")


def parse_jaspar(text: str, what: str = "<text>") -> list:
    """Motifs of JASPAR-format text: ``>ID [NAME]`` (the name defaults to the ID, as HOCOMOCO's files need),
    then the rows ``A|C|G|T [ n n ... ]`` in any order, the brackets optional."""
    out, head, rows = [], None, {}

    def close():
        if head is None:
            return
        if sorted(rows) != sorted(ALPHABET):
            raise ValueError(f"{what}: motif {head[0]} has rows {''.join(sorted(rows)) or 'none'}, not one each of A C G T")
        widths = {len(rows[a]) for a in ALPHABET}
        if len(widths) != 1 or 0 in widths:
            raise ValueError(f"{what}: motif {head[0]} has rows of {sorted(len(rows[a]) for a in ALPHABET)} counts")
        out.append(Motif(head[0], head[1], np.array([rows[a] for a in ALPHABET], np.float64).T.copy()))

    for ln in text.splitlines():
        if not ln.strip():
            continue
        if ln.startswith(">"):
            close()
            m = _HEADER.match(ln)
            if m is None:
                raise ValueError(f"{what}: header {ln!r} without an id")
            head, rows = (m.group(1), m.group(2) or m.group(1)), {}
            continue
        m = _ROW.match(ln)
        if m is None or head is None:
            raise ValueError(f"{what}: cannot read the line {ln!r}")
        letter = m.group(1).upper()
        if letter in rows:
            raise ValueError(f"{what}: motif {head[0]} has two {letter} rows")
        try:
            rows[letter] = [float(t) for t in m.group(2).split()]
        except ValueError:
            raise ValueError(f"{what}: motif {head[0]}: a count in {ln!r} is no number") from None
    close()
    return out


def read_jaspar(path: str) -> list:
    with open(path) as f:
        return parse_jaspar(f.read(), path)


def format_jaspar(motifs) -> str:
    """One motif after another: ``>ID NAME``, then ``A [%6.2f %6.2f ...]`` for A, C, G, T."""
    lines = []
    for m in motifs:
        lines.append(f">{m.id} {m.name}\n")
        counts = np.asarray(m.counts, np.float64)
        for b, letter in enumerate(ALPHABET):
            lines.append(f"{letter} [{' '.join('%6.2f' % v for v in counts[:, b])}]\n")
    return "".join(lines)


def read_jaspar_dir(directory: str) -> list:
    """One motif per ``*.jaspar`` file, the files in sorted order (cluster_by_pwm.py:43-49)."""
    out = []
    for path in sorted(glob.glob(f"{directory}/*.jaspar")):
        motif_list = read_jaspar(path)
        if len(motif_list) != 1:
            raise ValueError(f"more than one motif found in {path}" if motif_list else f"no motif found in {path}")
        out.append(motif_list[0])
    return out


def read_motif_file(path: str) -> list:
    """``--motif_file``: MEME text (``.meme``; counts = frequencies x nsites, name = the alternate id or
    the id) or JASPAR text."""
    if path.lower().endswith(".meme"):
        from .query_fimo_for_predictions import read_meme
        meme = read_meme(path)
        return [Motif(i, alt or i, np.asarray(f, np.float64) * float(n))
                for i, alt, f, n in zip(meme.ids, meme.alt_ids, meme.freqs, meme.nsites)]
    return read_jaspar(path)


# ---- stage 1 -----------------------------------------------------------------------------------

def select_motifs(assays, jaspar_motifs, hocomoco_motifs):
    """cluster_by_pwm.py:52-72.  ``assays``: the HGNC assay names of the kept marks.  Returns (the motifs
    to cluster, JASPAR's first, each source in its own order; the names found; the names looked for)."""
    included_motif_names = set(str(a).upper() for a in assays)
    motifs_found = set()
    cluster_motifs = []
    for motif in jaspar_motifs:
        if len(motif.name.split('::')) > 1:      # heterodimers
            continue
        tf_name = motif.name.upper()
        if tf_name in included_motif_names:
            motifs_found.add(tf_name)
            cluster_motifs.append(motif)
    for motif in hocomoco_motifs:
        tf_name = motif.name.split("_")[0].upper()
        if tf_name in included_motif_names:
            motifs_found.add(tf_name)
            cluster_motifs.append(motif)
    return cluster_motifs, motifs_found, included_motif_names


def kept_assays(features_path: str):
    """The HGNC assay names of the marks the reference keeps (cluster_by_pwm.py:32-40)."""
    from . import predict
    beluga_features_df = predict.read_features_table(features_path)
    keep_mask, hgnc_df = predict.get_keep_mask(beluga_features_df, no_tf_features=False, no_dnase_features=True,
                                               no_histone_features=True, no_pol2=True, intersect_with_lambert=True,
                                               return_hgnc_df=True)
    return hgnc_df[keep_mask]["Assay"]


# ---- stage 2 -----------------------------------------------------------------------------------

def _count_matrices(motifs):
    return [np.asarray(m.counts if isinstance(m, Motif) else m, np.float64) for m in motifs]


def frequencies(motifs, pseudo: float = 1.0):
    """``(freq float64 [sum w, 4], col_ptr int32 [M + 1])`` of count matrices [w, 4] (or :class:`Motif`),
    after the checks: at most 4096 motifs of 1..64 columns, finite non-negative counts, no all-zero column."""
    mats = _count_matrices(motifs)
    pseudo = float(pseudo)
    if not (np.isfinite(pseudo) and pseudo >= 0):
        raise ValueError(f"pseudo {pseudo!r} must be finite and not negative")
    if len(mats) > MAX_M:
        raise ValueError(f"{len(mats)} motifs; supported are at most {MAX_M}")
    for k, c in enumerate(mats):
        if c.ndim != 2 or c.shape[1] != 4:
            raise ValueError(f"motif {k}: counts of shape {c.shape}; expected [w, 4]")
        if not 1 <= c.shape[0] <= MAX_W:
            raise ValueError(f"motif {k}: width {c.shape[0]}; supported are 1..{MAX_W}")
        if not np.isfinite(c).all():
            raise ValueError(f"motif {k}: a count is NaN or infinite")
        if (c < 0).any():
            raise ValueError(f"motif {k}: a negative count")
        if not c.any(axis=1).all():
            raise ValueError(f"motif {k}: column {int(np.nonzero(~c.any(axis=1))[0][0])} is all zero")
    col_ptr = np.zeros(len(mats) + 1, np.int32)
    col_ptr[1:] = np.cumsum([c.shape[0] for c in mats])
    c = np.concatenate(mats) if mats else np.zeros((0, 4))
    total = ((c[:, 0] + c[:, 1]) + c[:, 2]) + c[:, 3]
    freq = (c + pseudo / 4) / (total + pseudo)[:, None]
    return np.ascontiguousarray(freq), col_ptr


def _n_of_condensed(length: int) -> int:
    n = int((1 + np.sqrt(1 + 8 * length)) // 2)
    if n * (n - 1) // 2 != length or n < 2:
        raise ValueError(f"{length} entries are not the pairs of n >= 2 points")
    return n


def compare(motifs, min_w: int = 5, pseudo: float = 1.0, device=None, timings=None) -> Comparison:
    """Every pair of motifs at its best alignment (one ``expecto_pwm_compare`` call).  ``motifs``: count
    matrices [w, 4] or :class:`Motif`.  ``timings``: a dict that receives the call's device time in ms
    (``compare_ms``), measured with events.  ``ValueError`` for bad input before the device is touched."""
    freq, col_ptr = frequencies(motifs, pseudo)
    if int(min_w) < 1:
        raise ValueError("min_w must be at least 1")
    from . import _lib
    torch = _lib.require_gpu("cluster_by_pwm")
    dev = _lib.device_of(device)
    M = len(col_ptr) - 1
    npair = M * (M - 1) // 2
    with torch.cuda.device(dev):
        d_freq, d_ptr = _lib.upload(freq, dev), _lib.upload(col_ptr, dev)
        f64 = [torch.empty(npair, dtype=torch.float64, device=dev) for _ in range(3)]
        i32 = [torch.empty(npair, dtype=torch.int32, device=dev) for _ in range(3)]
        timer = _lib.EventTimer(timings)
        timer.mark()
        _lib.call("expecto_pwm_compare", d_freq.data_ptr(), col_ptr.ctypes.data, d_ptr.data_ptr(), M, int(min_w),
                  *[t.data_ptr() for t in f64 + i32])
        timer.mark()
        out = [t.cpu().numpy() for t in f64 + i32]
        timer.set("compare_ms")
    return Comparison(*out)


def linkage(dist) -> Tree:
    """scipy's ``linkage(dist, method='average')`` of condensed distances, on the host."""
    D = np.array(dist, dtype=np.float64, order='C')
    if D.ndim != 1:
        raise ValueError("linkage: a condensed distance vector is 1-D")
    n = _n_of_condensed(D.size)
    children, heights, sizes = np.empty((n - 1, 2), np.int32), np.empty(n - 1, np.float64), np.empty(n - 1, np.int32)
    from . import _lib
    _lib.host_call("expecto_average_linkage", D.ctypes.data, n, children.ctypes.data, heights.ctypes.data,
                   sizes.ctypes.data)
    return Tree(children, heights, sizes)


def threshold_cut(tree, cor, ncor, min_cor: float = 0.6, min_ncor: float = 0.4) -> Cut:
    """The clusters of ``tree`` (a :class:`Tree` or its children array): the maximal merges whose own and
    whose descendants' mean cor and mean Ncor reach the thresholds."""
    children = np.ascontiguousarray(tree.children if isinstance(tree, Tree) else tree, np.int32)
    cor, ncor = np.ascontiguousarray(cor, np.float64), np.ascontiguousarray(ncor, np.float64)
    if children.ndim != 2 or children.shape[1] != 2:
        raise ValueError(f"threshold_cut: children of shape {children.shape}; expected [n - 1, 2]")
    n = children.shape[0] + 1
    if cor.shape != (n * (n - 1) // 2,) or ncor.shape != cor.shape:
        raise ValueError(f"threshold_cut: cor and ncor must hold the {n * (n - 1) // 2} pairs of {n} leaves")
    labels, mean_cor, mean_ncor = np.empty(n, np.int32), np.empty(n - 1, np.float64), np.empty(n - 1, np.float64)
    from . import _lib
    _lib.host_call("expecto_linkage_threshold_cut", children.ctypes.data, n, cor.ctypes.data, ncor.ctypes.data,
                   float(min_cor), float(min_ncor), labels.ctypes.data, mean_cor.ctypes.data, mean_ncor.ctypes.data)
    return Cut(labels, mean_cor, mean_ncor)


def cluster(motifs, cor: float = 0.6, ncor: float = 0.4, min_w: int = 5, pseudo: float = 1.0, device=None,
            timings=None) -> Clustering:
    """:func:`compare`, :func:`linkage` of its distances and :func:`threshold_cut`.  A single motif is one
    cluster with an empty tree."""
    comp = compare(motifs, min_w=min_w, pseudo=pseudo, device=device, timings=timings)
    if len(motifs) < 2:
        empty = np.empty(0, np.float64)
        return Clustering(comp, Tree(np.empty((0, 2), np.int32), empty, np.empty(0, np.int32)),
                          Cut(np.ones(len(motifs), np.int32), empty, empty))
    tree = linkage(comp.dist)
    return Clustering(comp, tree, threshold_cut(tree, comp.cor, comp.ncor, cor, ncor))


# ---- files -------------------------------------------------------------------------------------

def clusters_tab(names, labels) -> str:
    """``clusters_motif_names.tab``: one line ``cluster_k<TAB>name,name,...`` per cluster, k ascending."""
    members = {}
    for name, k in zip(names, labels):
        members.setdefault(int(k), []).append(str(name))
    return "".join(f"cluster_{k}\t{','.join(members[k])}\n" for k in sorted(members))


def pairwise_table(ids, comp: Comparison) -> str:
    M = len(ids)
    lines = ["id1\tid2\tcor\tNcor\tstrand\toffset\tw\n"]
    p = 0
    for i in range(M):
        for j in range(i + 1, M):
            lines.append(f"{ids[i]}\t{ids[j]}\t{float(comp.cor[p])!r}\t{float(comp.ncor[p])!r}\t"
                         f"{'DR'[int(comp.strand[p])]}\t{int(comp.offset[p])}\t{int(comp.width[p])}\n")
            p += 1
    return "".join(lines)


# ---- CLI ---------------------------------------------------------------------------------------

def build_parser():
    """The arguments of cluster_by_pwm.py:13-24, and those of the clustering stage."""
    parser = argparse.ArgumentParser(prog="python -m expecto_amd.cluster_by_pwm", description='Cluster features by PWM')
    parser.add_argument('--belugaFeatures', action="store", dest="belugaFeatures",
                        help="tsv file denoting Beluga features")
    parser.add_argument('--jaspar_motif_db', action="store", dest="jaspar_motif_db", help="JASPAR motif db path")
    parser.add_argument('--hocomoco_jaspar_motif_file', action="store", dest="hocomoco_jaspar_motif_file",
                        help="HOCOMOCO motifs file in JASPAR format")
    parser.add_argument('--cisbp2_meme_file', action="store", dest="cisbp2_meme_file",
                        help="CIS-BP 2 Homo sapiens meme file (ignored, as in the reference)")
    parser.add_argument('--motif_file', default=None, help="cluster these motifs (JASPAR or .meme); no selection")
    parser.add_argument('--no_cluster', action='store_true', help="stop after writing cluster_motifs.jaspar")
    parser.add_argument('--cor', type=float, default=0.6, help="least mean cor of a merge")
    parser.add_argument('--ncor', type=float, default=0.4, help="least mean Ncor of a merge")
    parser.add_argument('--min_w', type=int, default=5, help="least overlap of an alignment, in columns")
    parser.add_argument('--pseudo', type=float, default=1.0, help="pseudocount of a column")
    parser.add_argument('-o', dest="out_dir", type=str, default='temp_cluster_by_pwm', help='Output directory')
    return parser


def run(args):
    """One CLI run; returns ``(motifs, Clustering or None)``."""
    os.makedirs(args.out_dir, exist_ok=True)
    if args.motif_file is not None:
        cluster_motifs = read_motif_file(args.motif_file)
    else:
        for name in ("belugaFeatures", "jaspar_motif_db", "hocomoco_jaspar_motif_file"):
            if getattr(args, name) is None:
                raise ValueError(f"--{name} is required without --motif_file")
        assays = kept_assays(args.belugaFeatures)
        cluster_motifs, motifs_found, included = select_motifs(assays, read_jaspar_dir(args.jaspar_motif_db),
                                                               read_jaspar(args.hocomoco_jaspar_motif_file))
        print(f"Found {len(motifs_found)} motifs out of {len(included)} motifs in hgnc df")
    if not args.no_cluster:
        frequencies(cluster_motifs, args.pseudo)          # refuse before anything is written
    with open(f"{args.out_dir}/cluster_motifs.jaspar", "w") as out_file:
        print(format_jaspar(cluster_motifs), file=out_file)
    if args.no_cluster:
        return cluster_motifs, None
    if not cluster_motifs:
        raise ValueError("no motif to cluster")
    res = cluster(cluster_motifs, cor=args.cor, ncor=args.ncor, min_w=args.min_w, pseudo=args.pseudo)
    with open(f"{args.out_dir}/clusters_motif_names.tab", "w") as f:
        f.write(clusters_tab([m.name for m in cluster_motifs], res.labels))
    with open(f"{args.out_dir}/pairwise_compa.tsv", "w") as f:
        f.write(pairwise_table([m.id for m in cluster_motifs], res.comparison))
    np.savez(f"{args.out_dir}/tree.npz", children=res.tree.children, distances=res.tree.distances, sizes=res.tree.sizes,
             mean_cor=res.cut.mean_cor, mean_ncor=res.cut.mean_ncor)
    return cluster_motifs, res


def main(argv=None):
    return run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main(sys.argv[1:])
