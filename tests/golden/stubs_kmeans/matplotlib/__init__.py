"""Stand-in: cluster_and_viz.py draws a t-SNE scatter plot after clustering; here every call is a no-op."""
