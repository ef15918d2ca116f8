"""ExPecto expression models: xgboost ``gblinear`` boosters, read without xgboost.

The reference scores variant features with ``xgb.Booster.load_model(...).predict(DMatrix)``
(``predict.py:150-166``) on the models ``train.py:140-157`` writes (``booster='gblinear'``,
``objective='reg:linear'``, ``base_score`` 2, saved as ``*.save``; the pinned library is
``xgboost==0.7.post4``, ``requirements.txt``).  xgboost is not installed here, so this module
restates the published model formats and the gblinear prediction rule:

* legacy binary (``Booster.save_model`` of xgboost 0.7-0.90, the reference's ``.save``):
  optional ``binf`` magic; ``LearnerModelParam`` (136 B: f32 base_score, u32 num_feature,
  i32 num_class, i32 contain_extra_attrs, i32 contain_eval_metrics, 29 reserved i32);
  objective name and booster name as (u64 length, bytes); ``GBLinearModelParam`` (136 B:
  u32 num_feature, i32 num_output_group, 32 reserved i32); the weights as (u64 count,
  f32[count]) with ``w[f * groups + g]`` and the biases ``w[num_feature * groups + g]``;
  then, when contain_extra_attrs, the attribute pairs (ignored);
* JSON (``save_model('*.json')``, xgboost >= 1.0): ``learner.gradient_booster.model.weights``
  in the same order, ``learner.learner_model_param.base_score``;
* text dump (``dump_model``, ``train.py:158``): ``bias:`` / ``weight:`` sections; the dump
  holds no base_score, so it must be given (the reference's file names carry it:
  ``...basescore2...``).

Prediction (xgboost 0.7 ``GBLinear::Pred``): per row and output group, in float32,
``psum = bias + base_score``, then for every feature in column order
``psum += float32(x_f) * w_f`` (separate multiply and add, no FMA), dense rows (the
DMatrix of a dense numpy array keeps zeros).  ``predict`` runs that loop on the GPU
(``expecto_gblinear_predict``, one thread per row, features staged through LDS), reading
float64 feature rows directly (the DMatrix conversion is the kernel's first rounding).
Parity of the arithmetic against xgboost itself is unpinned (xgboost absent); the CLI
plumbing around it is pinned by running the reference ``predict.py`` (tests/golden).

Training (``train``; the reference's ``xgb.train`` of ``train.py:140-146`` and
``train_bootstrap.py:100-106``): xgboost 0.7 ``GBLinear::DoBoost`` plus the learner's round loop
as they run with ``nthread=1`` -- cyclic coordinate descent on weighted ridge / elastic-net
least squares, float32 state, double sums (DESIGN.md "Training gblinear models" restates every
step).  With more threads xgboost races on the gradient and is not reproducible, so the
single-thread order is the definition here.  Each round is one launch of
``expecto_gblinear_train_round``, one workgroup per model; a batch of models shares the
column-major float32 copy of ``X`` (``ColMatrix``).  As for ``predict``, parity against xgboost
itself is unpinned (xgboost absent): the tests hold the kernels to a numpy restatement of the
same steps, within the float32-vs-float64 noise of that restatement.
"""
from __future__ import annotations

import json
import struct
from dataclasses import dataclass, field

import numpy as np

TRAIN_MAX_ROWS = 24576              # EXPECTO_GBLINEAR_TRAIN_MAX_ROWS: rows one workgroup keeps on chip

_LEARNER_FMT = "<fIiii29i"          # LearnerModelParam, 136 bytes
_GBLINEAR_FMT = "<Ii32i"            # GBLinearModelParam, 136 bytes
assert struct.calcsize(_LEARNER_FMT) == 136 and struct.calcsize(_GBLINEAR_FMT) == 136


@dataclass
class GBLinear:
    """weights [num_feature, groups] f32, bias [groups] f32, base_score f32."""
    weights: np.ndarray
    bias: np.ndarray
    base_score: float
    objective: str = "reg:linear"
    attrs: dict = field(default_factory=dict)

    @property
    def num_feature(self) -> int:
        return int(self.weights.shape[0])

    @property
    def groups(self) -> int:
        return int(self.weights.shape[1])

    # -- formats ------------------------------------------------------------------------
    @classmethod
    def load(cls, path: str, base_score: float | None = None) -> "GBLinear":
        with open(path, "rb") as f:
            raw = f.read()
        head = raw.lstrip()[:1]
        if head == b"{":
            return cls._from_json(json.loads(raw.decode()))
        if raw.startswith(b"bias:") or raw.startswith(b"booster[0]:\nbias:"):
            return cls._from_dump(raw.decode(), base_score)
        return cls._from_legacy(raw)

    @classmethod
    def _from_legacy(cls, raw: bytes) -> "GBLinear":
        off = 4 if raw[:4] == b"binf" else 0
        if raw[:4] == b"bs64":
            raise ValueError("base64 xgboost models are not supported (nor by xgboost 0.7)")
        try:
            lp = struct.unpack_from(_LEARNER_FMT, raw, off)
        except struct.error as e:
            raise ValueError(f"not an xgboost model: {e}") from None
        base_score, num_feature, _num_class, extra_attrs = lp[0], lp[1], lp[2], lp[3]
        off += 136

        def read_str(o):
            (n,) = struct.unpack_from("<Q", raw, o)
            o += 8
            if n >= 0xFFFFFFFF:            # pre-0.6 layout: length in the high word + a gap
                o += 4
                n >>= 32
            return raw[o:o + n].decode(), o + n

        obj, off = read_str(off)
        gbm, off = read_str(off)
        if gbm != "gblinear":
            raise ValueError(f"booster {gbm!r} is not gblinear (ExPecto models are linear)")
        gp = struct.unpack_from(_GBLINEAR_FMT, raw, off)
        nf, groups = gp[0], gp[1]
        off += 136
        (count,) = struct.unpack_from("<Q", raw, off)
        off += 8
        if count != (nf + 1) * groups:
            raise ValueError(f"gblinear weight count {count} != (num_feature+1)*groups = {(nf + 1) * groups}")
        w = np.frombuffer(raw, dtype="<f4", count=count, offset=off).astype(np.float32)
        off += 4 * count
        attrs = {}
        if extra_attrs:
            (na,) = struct.unpack_from("<Q", raw, off)
            off += 8
            for _ in range(na):
                k, off = read_str(off)
                v, off = read_str(off)
                attrs[k] = v
        if num_feature and num_feature != nf:
            raise ValueError(f"learner num_feature {num_feature} != gblinear num_feature {nf}")
        w = w.reshape(nf + 1, groups)
        return cls(w[:nf].copy(), w[nf].copy(), float(np.float32(base_score)), obj, attrs)

    @classmethod
    def _from_json(cls, js: dict) -> "GBLinear":
        lrn = js["learner"]
        gb = lrn["gradient_booster"]
        if gb.get("name") != "gblinear":
            raise ValueError(f"booster {gb.get('name')!r} is not gblinear")
        mp = lrn["learner_model_param"]
        nf = int(mp["num_feature"])
        groups = max(1, int(mp.get("num_target", mp.get("num_class", 1)) or 1))
        w = np.asarray(gb["model"]["weights"], dtype=np.float32)
        if w.size != (nf + 1) * groups:
            raise ValueError("gblinear weight count does not match num_feature")
        w = w.reshape(nf + 1, groups)
        base = float(np.float32(float(str(mp["base_score"]).strip("[]"))))
        obj = lrn.get("objective", {}).get("name", "reg:linear")
        return cls(w[:nf].copy(), w[nf].copy(), base, obj)

    @classmethod
    def _from_dump(cls, text: str, base_score: float | None) -> "GBLinear":
        if base_score is None:
            raise ValueError("a gblinear text dump has no base_score: pass base_score=")
        lines = [l.strip() for l in text.splitlines() if l.strip() and not l.startswith("booster[")]
        bi, wi = lines.index("bias:"), lines.index("weight:")
        bias = np.array([float(x) for x in lines[bi + 1:wi]], dtype=np.float32)
        groups = bias.size
        w = np.array([float(x) for x in lines[wi + 1:]], dtype=np.float32).reshape(-1, groups)
        return cls(w, bias, float(np.float32(base_score)))

    def save_legacy(self, path: str) -> None:
        """Write the xgboost 0.7 binary layout described in the module docstring."""
        nf, g = self.weights.shape

        def wstr(s: str) -> bytes:
            b = s.encode()
            return struct.pack("<Q", len(b)) + b

        w = np.concatenate([self.weights.reshape(-1), self.bias.reshape(-1)]).astype("<f4")
        out = [b"binf", struct.pack(_LEARNER_FMT, np.float32(self.base_score), nf, 0, 0, 0, *([0] * 29)),
               wstr(self.objective), wstr("gblinear"), struct.pack(_GBLINEAR_FMT, nf, g, *([0] * 32)),
               struct.pack("<Q", w.size), w.tobytes()]
        with open(path, "wb") as f:
            f.write(b"".join(out))

    def save_dump(self, path: str) -> None:
        """Write xgboost's text dump (``Booster.dump_model`` of a gblinear model): ``booster[0]:``,
        ``bias:`` with one ``%g`` per group, ``weight:`` with one ``%g`` per weight."""
        lines = ["booster[0]:", "bias:"] + ["%g" % float(b) for b in self.bias.reshape(-1)]
        lines += ["weight:"] + ["%g" % float(w) for w in self.weights.reshape(-1)]
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")

    def dump_weights(self) -> np.ndarray:
        """The weights as the reference's interpretation step reads them
        (``predict_by_cluster.py:74-76``: ``float()`` of every weight line of ``model.get_dump()``):
        float64, at the ``%g`` precision of ``save_dump``."""
        return np.array([float("%g" % float(w)) for w in self.weights.reshape(-1)], dtype=np.float64)

    # -- scoring ------------------------------------------------------------------------
    def predict(self, X, cols=None, group: int = 0, out=None):
        """GPU gblinear margin of rows of X (float64 [n, ld] device tensor): feature j of a row
        is X[:, cols[j]] (cols: int32 device tensor or None = 0..num_feature-1)."""
        import torch

        from . import _lib

        lib = _lib.load()
        if X.dtype != torch.float64 or X.dim() != 2 or X.stride(1) != 1:
            raise RuntimeError("gblinear predict: X must be a float64 [n, ld] tensor with contiguous rows")
        n = X.shape[0]
        if cols is None:
            if X.shape[1] < self.num_feature:
                raise RuntimeError("gblinear predict: fewer columns than model features")
            cols = torch.arange(self.num_feature, dtype=torch.int32, device=X.device)
        if cols.numel() != self.num_feature:
            raise RuntimeError(f"model has {self.num_feature} features, {cols.numel()} columns given")
        w = torch.from_numpy(np.ascontiguousarray(self.weights[:, group])).to(X.device)
        init = float(np.float32(self.bias[group]) + np.float32(self.base_score))   # bias + base, in f32
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=X.device)
        _lib.check(lib.expecto_gblinear_predict(_lib.dptr(X), n, X.stride(0), _lib.dptr(cols.contiguous()),
                                                self.num_feature, _lib.dptr(w), float(init), _lib.dptr(out),
                                                _lib.stream_ptr()), "gblinear_predict")
        return out


# -- training -----------------------------------------------------------------------------------
class ColMatrix:
    """The training matrix as the kernels read it: float32 (the DMatrix rounding), column-major
    ``[F, ld]`` on the device, ``ld`` = n rounded up to 64 rows (zero padding).  Build it once and
    pass it to any number of ``train`` / ``predict_cols`` calls."""

    def __init__(self, X, device=None, chunk: int = 1024):
        import torch

        if isinstance(X, np.ndarray):
            X = torch.from_numpy(X)
        if X.dim() != 2:
            raise RuntimeError("gblinear train: X must be [n, F]")
        dev = torch.device(device) if device is not None else (
            X.device if X.is_cuda else torch.device("cuda", torch.cuda.current_device()))
        self.n, self.F = int(X.shape[0]), int(X.shape[1])
        self.ld = max(64, (self.n + 63) // 64 * 64)
        self.data = torch.zeros(max(self.F, 1), self.ld, dtype=torch.float32, device=dev)
        for c0 in range(0, self.F, chunk):            # a slab of columns at a time: no second full copy
            self.data[c0:c0 + chunk, :self.n] = X[:, c0:c0 + chunk].to(dev).to(torch.float32).T

    @property
    def device(self):
        return self.data.device


def _rows(v, n, what, dev):
    """[n] or [B, n] labels / weights -> (float32 device tensor, B or None, row stride)."""
    import torch

    t = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).to(dev).to(torch.float32).contiguous()
    if t.dim() == 1 and t.shape[0] == n:
        return t, None, 0
    if t.dim() == 2 and t.shape[1] == n:
        return t, int(t.shape[0]), n
    raise RuntimeError(f"gblinear train: {what} must be [n] or [B, n] with n = {n}")


def _batch(parts):
    """Common batch size of (tensor, B, stride) triples; None when all are single vectors."""
    sizes = {b for _, b, _ in parts if b is not None}
    if len(sizes) > 1:
        raise RuntimeError(f"gblinear train: batch sizes differ: {sorted(sizes)}")
    return sizes.pop() if sizes else None


def _rmse(lib, pred, y, h, n, B, out):
    from . import _lib

    _lib.check(lib.expecto_gblinear_rmse(_lib.dptr(pred), _lib.dptr(y[0]), y[2], _lib.dptr(h[0]) if h else None,
                                         h[2] if h else 0, n, B, _lib.dptr(out), _lib.stream_ptr()), "gblinear_rmse")


def predict_cols(X, models):
    """Margins of one ``GBLinear`` or a list of them on a ``ColMatrix``: float32 ``[n]`` or
    ``[B, n]`` device tensor, by the prediction rule above (``expecto_gblinear_predict_cols``)."""
    import torch

    from . import _lib

    lib = _lib.load()
    single = isinstance(models, GBLinear)
    ms = [models] if single else list(models)
    if any(m.num_feature != X.F or m.groups != 1 for m in ms):
        raise RuntimeError("gblinear predict_cols: single-group models with the matrix's feature count")
    if len({float(np.float32(m.base_score)) for m in ms}) > 1:
        raise RuntimeError("gblinear predict_cols: models of one call share base_score")
    w = np.stack([np.concatenate([m.weights[:, 0], m.bias[:1]]).astype(np.float32) for m in ms]) if ms else \
        np.zeros((0, X.F + 1), np.float32)
    out = torch.empty(len(ms), X.n, dtype=torch.float32, device=X.device)
    if ms:
        _predict_cols(lib, X, torch.from_numpy(w).to(X.device), float(ms[0].base_score), out)
    return out[0] if single else out


def _predict_cols(lib, X, w, base_score, out):
    from . import _lib

    _lib.check(lib.expecto_gblinear_predict_cols(_lib.dptr(X.data), X.ld, X.n, X.F, int(w.shape[0]), _lib.dptr(w),
                                                 float(base_score), _lib.dptr(out), _lib.stream_ptr()),
               "gblinear_predict_cols")


def train(X, y, weight=None, *, num_round=100, eta=0.01, lambda_=100.0, alpha=0.0, lambda_bias=0.0,
          base_score=2.0, evals=()):
    """Train gblinear / reg:linear models on the GPU (module docstring: "Training").

    X: ``[n, F]`` array / tensor, or a ``ColMatrix`` (reusable across calls).  y, weight: ``[n]``,
    or ``[B, n]`` for a batch of B models sharing X (a bootstrap replicate is its draw counts as
    weight).  evals: ``(X_e, y_e)`` or ``(X_e, y_e, weight_e)`` tuples, y_e ``[n_e]`` or ``[B, n_e]``.
    Returns ``(models, history)``: a ``GBLinear`` and a float64 ``[num_round, 1 + len(evals)]``
    array (the train rmse, then each eval set's, after every round), or for a batch a list of
    ``GBLinear`` and ``[B, num_round, 1 + len(evals)]``."""
    import torch

    from . import _lib

    lib = _lib.load()
    Xc = X if isinstance(X, ColMatrix) else ColMatrix(X)
    dev, n, F = Xc.device, Xc.n, Xc.F
    yt = _rows(y, n, "y", dev)
    ht = _rows(weight, n, "weight", dev) if weight is not None else None
    ev = []
    for e in evals:
        Xe = e[0] if isinstance(e[0], ColMatrix) else ColMatrix(e[0], device=dev)
        if Xe.F != F:
            raise RuntimeError("gblinear train: an eval set has another feature count")
        ev.append((Xe, _rows(e[1], Xe.n, "eval y", dev),
                   _rows(e[2], Xe.n, "eval weight", dev) if len(e) > 2 and e[2] is not None else None))
    Bq = _batch([yt] + ([ht] if ht else []) + [p for _, ye, he in ev for p in ([ye] + ([he] if he else []))])
    B = Bq or 1
    num_round = int(num_round)
    w = torch.zeros(B, F + 1, dtype=torch.float32, device=dev)
    sh = torch.empty(B, max(F, 1), dtype=torch.float64, device=dev)
    pred = torch.empty(B, n, dtype=torch.float32, device=dev)
    hist = torch.zeros(max(num_round, 1), 1 + len(ev), B, dtype=torch.float64, device=dev)
    epred = [torch.empty(B, Xe.n, dtype=torch.float32, device=dev) for Xe, _, _ in ev]
    base = float(np.float32(base_score))
    for r in range(num_round):
        # the round's own predict pass is the train prediction of the weights round r-1 left
        _lib.check(lib.expecto_gblinear_train_round(
            _lib.dptr(Xc.data), Xc.ld, n, F, B, _lib.dptr(yt[0]), yt[2], _lib.dptr(ht[0]) if ht else None,
            ht[2] if ht else 0, _lib.dptr(w), _lib.dptr(sh), int(r == 0), float(eta), float(lambda_), float(alpha),
            float(lambda_bias), base, _lib.dptr(pred) if r > 0 else None, _lib.stream_ptr()), "gblinear_train_round")
        if r > 0 and n > 0:
            _rmse(lib, pred, yt, ht, n, B, hist[r - 1, 0])
        for k, (Xe, ye, he) in enumerate(ev):
            if Xe.n > 0:
                _predict_cols(lib, Xe, w, base, epred[k])
                _rmse(lib, epred[k], ye, he, Xe.n, B, hist[r, 1 + k])
    if num_round > 0 and n > 0:
        _predict_cols(lib, Xc, w, base, pred)
        _rmse(lib, pred, yt, ht, n, B, hist[num_round - 1, 0])
    wh = w.cpu().numpy()
    history = hist[:num_round].permute(2, 0, 1).contiguous().cpu().numpy()
    models = [GBLinear(wh[m, :F].reshape(F, 1).copy(), wh[m, F:].copy(), base) for m in range(B)]
    if Bq is None:
        return models[0], history[0]
    return models, history
