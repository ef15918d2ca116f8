"""Stand-in: cluster_analysis_with_fimo.py draws three line plots; here every call is a no-op."""
