"""Stand-in: the plotting calls of predict_by_cluster_rsat.py:406-419 as no-ops."""


def _noop(*a, **k):
    return None


figure = bar = title = legend = tight_layout = savefig = show = close = Rectangle = _noop
