"""Stand-in: the plotting calls of cluster_and_viz.py:49-67 as no-ops."""


def _noop(*a, **k):
    return None


figure = plot = scatter = show = _noop
