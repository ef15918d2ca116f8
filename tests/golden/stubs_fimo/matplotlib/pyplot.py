"""Stand-in: the plotting calls of cluster_analysis_with_fimo.py:66-122 as no-ops."""


def _noop(*a, **k):
    return None


def __getattr__(name):
    return _noop
