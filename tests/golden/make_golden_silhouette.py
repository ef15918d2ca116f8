"""Record sklearn's silhouette on the three inputs of tests/silhouette_ref.py (CPU; needs scipy and
scikit-learn):

    python tests/golden/make_golden_silhouette.py

For each input, tests/golden/silhouette/<name>.npz holds, for every k in 2..n-1, the labels of
``AgglomerativeClustering(n_clusters=k).fit(X)``, ``silhouette_samples(squareform(pdist(X)), labels,
metric='precomputed')`` and ``silhouette_score`` of the same call.  The tests compare bits, where
sklearn is not installed too.

It also prints, per input, the largest difference over k between that score and the reference's
literal ``silhouette_score(X, labels)`` (``metric='euclidean'``: sklearn's Gram-form distances).  That
number is a property of sklearn's two routes; it is recorded in DESIGN.md and asserted nowhere."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import silhouette_ref  # noqa: E402


def main():
    import sklearn
    from scipy.spatial.distance import pdist, squareform
    from sklearn.cluster import AgglomerativeClustering
    from sklearn.metrics import silhouette_samples, silhouette_score

    out_dir = os.path.join(HERE, "silhouette")
    os.makedirs(out_dir, exist_ok=True)
    for name, make in silhouette_ref.INPUTS.items():
        X = make()
        n = X.shape[0]
        D = squareform(pdist(X))
        ks = np.arange(2, n)
        labels = np.stack([AgglomerativeClustering(n_clusters=int(k)).fit(X).labels_ for k in ks])
        samples = np.stack([silhouette_samples(D, lab, metric="precomputed") for lab in labels])
        scores = np.array([silhouette_score(D, lab, metric="precomputed") for lab in labels])
        literal = np.array([silhouette_score(X, lab) for lab in labels])
        np.savez_compressed(os.path.join(out_dir, name + ".npz"), ks=ks, labels=labels.astype(np.int16),
                            samples=samples, scores=scores)
        print(f"{name}: n = {n}, k = 2..{n - 1}, sklearn {sklearn.__version__}; "
              f"max |precomputed - euclidean route| of the score = {np.abs(scores - literal).max():.3g}, "
              f"argmax {ks[np.argmax(scores)]} vs {ks[np.argmax(literal)]}")


if __name__ == "__main__":
    main()
