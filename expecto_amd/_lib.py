"""ctypes binding of the C-ABI in include/expecto_hip.h (libexpecto_hip.so, gfx950).

The library is built in-tree (``python -m expecto_amd.build`` or
``__graft_entry__.build()``).  There is NO CPU fallback: if the library is missing or
fails to load, every product entry point raises ``RuntimeError``.

torch is imported before the library so that the HIP runtime torch already loaded
(soname ``libamdhip64.so.7``) is the one the library binds to: device pointers and
streams are then shared with torch tensors.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libexpecto_hip.so")

c_f32p = ctypes.POINTER(ctypes.c_float)
c_f64p = ctypes.POINTER(ctypes.c_double)
c_u8p = ctypes.POINTER(ctypes.c_uint8)
c_i64p = ctypes.POINTER(ctypes.c_longlong)
c_i32p = ctypes.POINTER(ctypes.c_int)
c_vp = ctypes.c_void_p

# name -> (restype, argtypes); must match include/expecto_hip.h exactly.
SIGNATURES = {
    "expecto_beluga_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(c_vp), ctypes.c_int, c_vp,
                                             ctypes.POINTER(c_vp)]),
    "expecto_beluga_destroy": (None, [c_vp]),
    "expecto_beluga_device_bytes": (ctypes.c_size_t, [c_vp]),
    "expecto_beluga_conv2_table_active": (ctypes.c_int, [c_vp, c_i32p]),
    "expecto_beluga_set_fc1_role": (ctypes.c_int, [c_vp, ctypes.c_int]),
    "expecto_beluga_forward_onehot": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, c_vp, c_vp]),
    "expecto_beluga_forward_codes": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_longlong, ctypes.c_int,
                                                    c_vp, c_vp]),
    "expecto_beluga_forward_segments": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_longlong,
                                                       ctypes.c_int, c_vp, c_vp, c_vp, ctypes.c_int, c_vp, c_vp]),
    "expecto_gather_segments": (ctypes.c_int, [c_vp, ctypes.c_longlong, c_vp, ctypes.c_int, ctypes.c_int, c_vp,
                                               c_vp, c_vp, c_vp]),
    "expecto_beluga_forward_pairs": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_longlong, c_vp,
                                                    ctypes.c_int, c_vp, c_vp, ctypes.c_longlong, c_vp]),
    "expecto_beluga_forward_segment_pairs": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int,
                                                            ctypes.c_longlong, ctypes.c_int, c_vp, c_vp, c_vp,
                                                            ctypes.c_int, c_vp, c_vp, ctypes.c_longlong, c_vp]),
    "expecto_beluga_set_precision": (ctypes.c_int, [c_vp, ctypes.c_int]),
    "expecto_beluga_get_precision": (ctypes.c_int, [c_vp]),
    "expecto_beluga_set_f16_target": (ctypes.c_int, [c_vp, ctypes.c_int]),
    "expecto_beluga_f16_fallbacks": (ctypes.c_longlong, [c_vp, c_i32p]),
    "expecto_beluga_set_overflow_check": (ctypes.c_int, [c_vp, ctypes.c_int]),
    "expecto_beluga_overflow_pending": (ctypes.c_int, [c_vp, c_vp]),
    "expecto_beluga_overflow_take": (ctypes.c_int, [c_vp, c_vp, c_vp]),
    "expecto_beluga_count_fallback": (ctypes.c_int, [c_vp]),
    "expecto_beluga_set_profiling": (ctypes.c_int, [c_vp, ctypes.c_int]),
    "expecto_beluga_layer_times": (ctypes.c_int, [c_vp, c_f64p, c_i64p, c_f64p, ctypes.c_int]),
    "expecto_beluga_main_launches": (ctypes.c_int, [c_vp, ctypes.c_int, c_i64p, c_f64p, c_i64p, c_f64p]),
    "expecto_variant_windows": (ctypes.c_int, [c_vp, ctypes.c_longlong, c_vp, c_vp, c_vp, ctypes.c_int, c_vp,
                                               ctypes.c_int, c_vp, c_vp]),
    "expecto_indel_windows": (ctypes.c_int, [c_vp, ctypes.c_longlong, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                             ctypes.c_int, c_vp, c_vp]),
    "expecto_tss_windows": (ctypes.c_int, [c_vp, ctypes.c_longlong, c_vp, c_vp, ctypes.c_int, c_vp, ctypes.c_int,
                                           c_vp, c_vp]),
    "expecto_diff": (ctypes.c_int, [c_vp, c_vp, ctypes.c_longlong, c_vp, c_vp]),
    "expecto_fwd_rc_average": (ctypes.c_int, [c_vp, ctypes.c_int, ctypes.c_int, c_vp, c_vp]),
    "expecto_tss_reduce": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, c_vp]),
    "expecto_variant_reduce": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              c_vp, c_vp]),
    "expecto_variant_reduce_lut": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                  c_vp, ctypes.c_int, c_vp, c_vp]),
    "expecto_variant_contrib": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               c_vp, ctypes.c_int, c_vp, ctypes.c_int, c_vp, ctypes.c_int, c_vp, c_vp,
                                               ctypes.c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "expecto_gblinear_predict": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_longlong, c_vp, ctypes.c_int,
                                                c_vp, ctypes.c_float, c_vp, c_vp]),
    "expecto_gblinear_train_round": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                    c_vp, ctypes.c_longlong, c_vp, ctypes.c_longlong, c_vp, c_vp,
                                                    ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                                    ctypes.c_double, ctypes.c_float, c_vp, c_vp]),
    "expecto_gblinear_train_round_hp": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                                       ctypes.c_int, c_vp, ctypes.c_longlong, c_vp, ctypes.c_longlong,
                                                       c_vp, c_vp, ctypes.c_int, c_vp, ctypes.c_float, c_vp, c_vp]),
    "expecto_gblinear_predict_cols": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                                     ctypes.c_int, c_vp, ctypes.c_float, c_vp, c_vp]),
    "expecto_gblinear_rmse": (ctypes.c_int, [c_vp, c_vp, ctypes.c_longlong, c_vp, ctypes.c_longlong, ctypes.c_int,
                                             ctypes.c_int, c_vp, c_vp]),
    "expecto_shift_reduce": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            c_vp, c_vp]),
    "expecto_pairwise_euclidean": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
                                                  c_vp, c_vp]),
    "expecto_ward_linkage": (ctypes.c_int, [c_vp, ctypes.c_int, c_vp, c_vp, c_vp]),
    "expecto_square_distances": (ctypes.c_int, [c_vp, ctypes.c_longlong, c_vp, c_vp]),
    "expecto_silhouette_node_sums": (ctypes.c_int, [c_vp, ctypes.c_int, ctypes.c_longlong, c_vp, c_vp, c_vp,
                                                    ctypes.c_longlong, c_vp, c_vp]),
    "expecto_silhouette_cuts": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_longlong, c_vp, c_vp, c_vp, c_vp,
                                               c_vp, ctypes.c_longlong, c_vp, c_vp]),
    "expecto_tfidf_stats": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_longlong, c_vp, ctypes.c_int, c_vp, c_vp,
                                           c_vp]),
    "expecto_tfidf_gram_parts": (ctypes.c_int, [ctypes.c_int, ctypes.c_longlong]),
    "expecto_tfidf_gram_workspace": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_longlong]),
    "expecto_tfidf_gram": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_longlong, c_vp, ctypes.c_int, c_vp, c_vp,
                                          c_vp, ctypes.c_size_t, c_vp]),
    "expecto_tfidf_project": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_longlong, c_vp, ctypes.c_int, c_vp,
                                             c_vp, ctypes.c_int, c_vp, ctypes.c_longlong, c_vp]),
    "expecto_tfidf_transform_parts": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_longlong]),
    "expecto_tfidf_transform_workspace": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_longlong]),
    "expecto_tfidf_transform": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_longlong, c_vp, ctypes.c_int, c_vp,
                                               c_vp, ctypes.c_longlong, ctypes.c_int, c_vp, c_vp, ctypes.c_size_t,
                                               c_vp]),
    "expecto_kmeans_workspace": (ctypes.c_size_t, [ctypes.c_longlong] * 5),
    "expecto_kmeans_plusplus": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
                                               ctypes.c_longlong, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.c_size_t,
                                               c_vp]),
    "expecto_kmeans_lloyd": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
                                            ctypes.c_longlong, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                            ctypes.c_size_t, c_vp]),
    "expecto_tsne_workspace": (ctypes.c_size_t, [ctypes.c_longlong]),
    "expecto_tsne_affinities": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
                                               ctypes.c_double, c_vp, c_vp, c_vp, c_vp, ctypes.c_size_t, c_vp]),
    "expecto_tsne_descend": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_double, c_vp, c_vp, c_vp,
                                            ctypes.c_double, ctypes.c_double, ctypes.c_longlong, ctypes.c_int, c_vp,
                                            c_vp, ctypes.c_size_t, c_vp]),
    "expecto_knn_jaccard": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
                                           ctypes.c_longlong, c_vp, c_vp, c_vp]),
    "expecto_louvain_workspace": (ctypes.c_size_t, [ctypes.c_longlong] * 3),
    "expecto_louvain": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
                                       c_vp, c_vp, ctypes.c_longlong, ctypes.c_longlong, c_vp, c_vp, c_vp, c_vp,
                                       ctypes.c_size_t, c_vp]),
    "expecto_cluster_enrich_workspace": (ctypes.c_size_t, [ctypes.c_longlong] * 2),
    "expecto_cluster_enrich": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, c_vp,
                                              ctypes.c_longlong, c_vp, c_vp, c_vp, ctypes.c_longlong, c_vp, c_vp,
                                              ctypes.c_longlong, c_vp, ctypes.c_longlong, c_vp, ctypes.c_longlong,
                                              c_vp, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, c_vp,
                                              c_vp, c_vp, c_vp, c_vp, ctypes.c_size_t, c_vp]),
    "expecto_hypergeom_sf": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.c_longlong, c_vp, c_vp]),
    "expecto_pwm_pvalues": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_longlong, c_vp, c_vp, c_vp, ctypes.c_longlong,
                                           c_vp]),
    "expecto_pwm_scan": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, c_vp, c_vp, c_vp,
                                        c_vp, ctypes.c_longlong, c_vp, c_vp, ctypes.c_longlong, c_vp, c_vp, c_vp, c_vp,
                                        c_vp]),
    "expecto_pwm_compare": (ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_longlong, ctypes.c_int, c_vp, c_vp, c_vp, c_vp,
                                           c_vp, c_vp, c_vp]),
    "expecto_average_linkage": (ctypes.c_int, [c_vp, ctypes.c_int, c_vp, c_vp, c_vp]),
    "expecto_linkage_threshold_cut": (ctypes.c_int, [c_vp, ctypes.c_int, c_vp, c_vp, ctypes.c_double, ctypes.c_double,
                                                     c_vp, c_vp, c_vp]),
    "expecto_rank2_f32": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, c_vp, c_vp]),
    "expecto_rank2_f64": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, c_vp, c_vp]),
    "expecto_model_metrics": (ctypes.c_int, [c_vp, ctypes.c_longlong, c_vp, ctypes.c_longlong, c_vp, c_vp,
                                             ctypes.c_int, ctypes.c_int, c_vp, c_vp]),
    "expecto_bootstrap_coef_stats": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, c_vp, c_vp,
                                                    c_vp, c_vp, c_vp, c_vp]),
    "expecto_ism_variants": (ctypes.c_int, [c_vp, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, c_vp, c_vp, c_vp,
                                            c_vp, c_vp]),
    "expecto_ism_score": (ctypes.c_int, [c_vp, c_vp, ctypes.c_longlong, c_vp, ctypes.c_int, c_vp, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, c_vp, ctypes.c_int, c_vp, ctypes.c_int, c_vp, c_vp,
                                         ctypes.c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "expecto_ism_summary": (ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_vp]),
    "expecto_ecdf_tail_counts": (ctypes.c_int, [c_vp, ctypes.c_int, ctypes.c_int, c_vp, c_vp, ctypes.c_int, c_vp,
                                                ctypes.c_longlong, ctypes.c_int, c_vp, c_vp]),
    "expecto_ecdf_summary": (ctypes.c_int, [c_vp, ctypes.c_int, ctypes.c_int, c_vp, ctypes.c_int, ctypes.c_int, c_vp,
                                            c_vp, c_vp, c_vp, c_vp]),
    "expecto_last_error": (ctypes.c_char_p, []),
    "expecto_version": (ctypes.c_char_p, []),
}

STRAND_FWD, STRAND_RC, STRAND_BOTH = 0, 1, 2
PRECISION_FP32, PRECISION_BF16X6, PRECISION_F16X3 = 0, 1, 2
PRECISIONS = {"fp32": PRECISION_FP32, "bf16x6": PRECISION_BF16X6, "f16x3": PRECISION_F16X3}
_BASE_LAYERS = ("conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "fc1", "fc1_reduce", "fc2")
# expecto_beluga_layer_times slots: the layers of every forward, then their alt-delta launches
LAYER_NAMES = _BASE_LAYERS + tuple(f"{n}_delta" for n in _BASE_LAYERS)
N_LAYERS = len(LAYER_NAMES)

_lib = None


def load(path: str = LIB_PATH):
    """Load (once) and return the ctypes library; raise RuntimeError if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  -- bind to torch's HIP runtime (see module docstring)

    if not os.path.exists(path):
        raise RuntimeError(f"HIP library {path} not built: run `python -m expecto_amd.build` "
                           "(there is no CPU fallback)")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = _lib.expecto_last_error().decode() if _lib is not None else ""
        raise RuntimeError(f"{what} failed (status {status}): {msg}")


def stream_ptr(stream=None) -> int:
    import torch

    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def dptr(t) -> int:
    """Device pointer of a CUDA (HIP) tensor; fails loudly on CPU tensors."""
    if not t.is_cuda:
        raise RuntimeError("expecto_amd kernels need device (HIP) tensors; there is no CPU path")
    return int(t.data_ptr())


# ---- the device-call layer of the analysis modules (INTEGRATION.md "Binding helpers") ----------

def require_gpu(module: str, what: str = ""):
    """torch, or the RuntimeError of a module that has no CPU path."""
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError(f"expecto_amd.{module} needs a GPU (HIP){what}; there is no CPU path")
    return torch


def device_of(device=None):
    """The given device as a ``torch.device``, or else the current HIP device."""
    import torch

    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def call(name: str, *args, what: str | None = None) -> None:
    """``name(*args, stream)`` on torch's current stream; RuntimeError with the library's message on a
    non-zero status.  ``what``: the label of the message where a call site's differs from ``name``."""
    lib = load()
    st = getattr(lib, name)(*args, stream_ptr())
    if st != 0:
        raise RuntimeError(f"{what or name} failed (status {st}): {lib.expecto_last_error().decode()}")


def host_call(name: str, *args, prefix: bool = True) -> None:
    """``name(*args)`` of an entry point that takes no stream; ValueError with the library's message,
    after ``name: `` unless ``prefix`` is false."""
    lib = load()
    if getattr(lib, name)(*args) != 0:
        msg = lib.expecto_last_error().decode()
        raise ValueError(f"{name}: {msg}" if prefix else msg)


def upload(array, dev):
    """A host array as a tensor on ``dev``."""
    import numpy as np
    import torch

    return torch.from_numpy(np.ascontiguousarray(array)).to(dev)


def workspace(nbytes: int, dev):
    """A float64 tensor of at least ``nbytes`` bytes on ``dev``."""
    import torch

    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)


class EventTimer:
    """Event-timed device milliseconds for a ``timings`` dict; with ``timings`` None every method does
    nothing and no event exists.  ``mark()`` records an event on the current stream; interval ``i`` lies
    between marks ``i`` and ``i + 1`` and must have completed (a copy to the host, or ``mark(sync=True)``)
    before ``set`` or ``add`` reads it."""

    def __init__(self, timings):
        self.timings, self.events = timings, []

    def mark(self, sync: bool = False) -> None:
        if self.timings is None:
            return
        import torch

        self.events.append(torch.cuda.Event(enable_timing=True))
        self.events[-1].record()
        if sync:
            self.events[-1].synchronize()

    def set(self, key: str, i: int = 0) -> None:
        if self.timings is not None:
            self.timings[key] = self.events[i].elapsed_time(self.events[i + 1])

    def add(self, key: str, i: int = 0) -> None:
        if self.timings is not None:
            self.timings[key] = self.timings.get(key, 0.0) + self.events[i].elapsed_time(self.events[i + 1])
