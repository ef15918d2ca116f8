"""Stand-in: a colour map with the 12 entries of Set3 (predict_by_cluster_rsat.py:408-409)."""


class _Cmap:
    colors = tuple((i / 12.0, i / 12.0, i / 12.0) for i in range(12))


def get_cmap(*a, **k):
    return _Cmap()
