"""Stand-in: predict_by_cluster_rsat.py draws bar plots after its tables; here every call is a no-op."""
