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

Choosing the penalties (``cv``, ``CVResult``; DESIGN.md "Cross-validated grid"): ``eta``,
``lambda_``, ``alpha`` and ``lambda_bias`` may differ per model of a batch
(``expecto_gblinear_train_round_hp`` reads a row of four doubles per model), so a grid of
penalties times K folds is one batch over one ``ColMatrix``.  A fold's held-out rows stay in the
matrix at weight zero, and the predictions each round starts from give its train and held-out
rmse without another pass over X.
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

        if X.dtype != torch.float64 or X.dim() != 2 or X.stride(1) != 1:
            raise RuntimeError("gblinear predict: X must be a float64 [n, ld] tensor with contiguous rows")
        n = X.shape[0]
        if cols is None:
            if X.shape[1] < self.num_feature:
                raise RuntimeError("gblinear predict: fewer columns than model features")
            cols = torch.arange(self.num_feature, dtype=torch.int32, device=X.device)
        if cols.numel() != self.num_feature:
            raise RuntimeError(f"model has {self.num_feature} features, {cols.numel()} columns given")
        w = _lib.upload(self.weights[:, group], X.device)
        init = float(np.float32(self.bias[group]) + np.float32(self.base_score))   # bias + base, in f32
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=X.device)
        _lib.call("expecto_gblinear_predict", _lib.dptr(X), n, X.stride(0), _lib.dptr(cols.contiguous()),
                  self.num_feature, _lib.dptr(w), float(init), _lib.dptr(out), what="gblinear_predict")
        return out


# -- training -----------------------------------------------------------------------------------
class ColMatrix:
    """The training matrix as the kernels read it: float32 (the DMatrix rounding), column-major
    ``[F, ld]`` on the device, ``ld`` = n rounded up to 64 rows (zero padding).  Build it once and
    pass it to any number of ``train`` / ``predict_cols`` calls."""

    def __init__(self, X, device=None, chunk: int = 1024):
        import torch

        from . import _lib

        if isinstance(X, np.ndarray):
            X = torch.from_numpy(X)
        if X.dim() != 2:
            raise RuntimeError("gblinear train: X must be [n, F]")
        dev = _lib.device_of(X.device if device is None and X.is_cuda else device)
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


def _rmse(pred, y, h, n, B, out):
    from . import _lib

    _lib.call("expecto_gblinear_rmse", _lib.dptr(pred), _lib.dptr(y[0]), y[2], _lib.dptr(h[0]) if h else None,
              h[2] if h else 0, n, B, _lib.dptr(out), what="gblinear_rmse")


def predict_cols(X, models):
    """Margins of one ``GBLinear`` or a list of them on a ``ColMatrix``: float32 ``[n]`` or
    ``[B, n]`` device tensor, by the prediction rule above (``expecto_gblinear_predict_cols``)."""
    import torch

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
        _predict_cols(X, torch.from_numpy(w).to(X.device), float(ms[0].base_score), out)
    return out[0] if single else out


def _predict_cols(X, w, base_score, out):
    from . import _lib

    _lib.call("expecto_gblinear_predict_cols", _lib.dptr(X.data), X.ld, X.n, X.F, int(w.shape[0]), _lib.dptr(w),
              float(base_score), _lib.dptr(out), what="gblinear_predict_cols")


_HYPER = ("eta", "lambda_", "alpha", "lambda_bias")


def _hyper(eta, lambda_, alpha, lambda_bias):
    """The four hyper-parameters, each a float or a length-B sequence -> ``(hyper, B)``: a tuple of
    four floats and None when all are floats, else a float64 ``[B, 4]`` array (a float serves every
    model).  Host only.  ValueError for a value that is not finite or a negative ``lambda_``,
    ``alpha`` or ``lambda_bias``; RuntimeError for sequences of different lengths."""
    vals = [np.asarray(v, dtype=np.float64) for v in (eta, lambda_, alpha, lambda_bias)]
    for name, v in zip(_HYPER, vals):
        if v.ndim > 1:
            raise ValueError(f"gblinear train: {name} must be a float or a length-B sequence")
        if not np.isfinite(v).all():
            raise ValueError(f"gblinear train: {name} must be finite")
        if name != "eta" and (v < 0).any():
            raise ValueError(f"gblinear train: {name} must be >= 0")
    sizes = {int(v.shape[0]) for v in vals if v.ndim == 1}
    if not sizes:
        return tuple(float(v) for v in vals), None
    if len(sizes) > 1:
        raise RuntimeError(f"gblinear train: batch sizes differ: {sorted(sizes)} (hyper-parameter sequences)")
    B = sizes.pop()
    return np.ascontiguousarray(np.stack([np.broadcast_to(v, (B,)) for v in vals], 1)), B


def _part(p, c0, c1):
    """Models c0..c1-1 of a (tensor, B, stride) triple; a shared vector serves every chunk."""
    return p if p is None or p[1] is None else (p[0][c0:c1], c1 - c0, p[2])


def _round(Xc, y, h, w, sh, first, hyper, base, pred):
    """One round of the models of ``w``: ``hyper`` is a tuple of four floats for all of them
    (``expecto_gblinear_train_round``) or a float64 ``[b, 4]`` device tensor, a row per model
    (``expecto_gblinear_train_round_hp``)."""
    from . import _lib

    head = (_lib.dptr(Xc.data), Xc.ld, Xc.n, Xc.F, int(w.shape[0]), _lib.dptr(y[0]), y[2],
            _lib.dptr(h[0]) if h else None, h[2] if h else 0, _lib.dptr(w), _lib.dptr(sh), int(first))
    tail = (base, _lib.dptr(pred) if pred is not None else None)
    if isinstance(hyper, tuple):
        _lib.call("expecto_gblinear_train_round", *head, *hyper, *tail, what="gblinear_train_round")
    else:
        _lib.call("expecto_gblinear_train_round_hp", *head, _lib.dptr(hyper), *tail, what="gblinear_train_round")


def _fit(Xc, y, h, hyper, w, num_round, base, train_pred, after_round=None):
    """``num_round`` rounds of the models of ``w`` (in place).  ``train_pred(r, pred)`` is called with
    the train predictions after round r (0-based): for every round but the last they are what the
    next round's own predict pass writes, so only the last costs a pass over X.
    ``after_round(r)`` is called once round r has updated ``w``."""
    import torch

    b, n = int(w.shape[0]), Xc.n
    sh = torch.empty(b, max(Xc.F, 1), dtype=torch.float64, device=w.device)
    pred = torch.empty(b, n, dtype=torch.float32, device=w.device)
    for r in range(num_round):
        _round(Xc, y, h, w, sh, r == 0, hyper, base, pred if r > 0 else None)
        if r > 0 and n > 0:
            train_pred(r - 1, pred)
        if after_round is not None:
            after_round(r)
    if num_round > 0 and n > 0:
        _predict_cols(Xc, w, base, pred)
        train_pred(num_round - 1, pred)


def train(X, y, weight=None, *, num_round=100, eta=0.01, lambda_=100.0, alpha=0.0, lambda_bias=0.0,
          base_score=2.0, evals=(), chunk=256):
    """Train gblinear / reg:linear models on the GPU (module docstring: "Training").

    X: ``[n, F]`` array / tensor, or a ``ColMatrix`` (reusable across calls).  y, weight: ``[n]``,
    or ``[B, n]`` for a batch of B models sharing X (a bootstrap replicate is its draw counts as
    weight).  evals: ``(X_e, y_e)`` or ``(X_e, y_e, weight_e)`` tuples, y_e ``[n_e]`` or ``[B, n_e]``.
    eta, lambda_, alpha, lambda_bias: a float each, or a length-B sequence giving every model of
    the batch its own value (any sequence makes the call a batch of that B; y, weight and the eval
    sets may still be single vectors, shared by all models).  All must be finite and lambda_, alpha,
    lambda_bias >= 0.  chunk: a batch is trained in successive launches of at most ``chunk`` models
    (256 workgroups fill the device); the results do not depend on it.
    Returns ``(models, history)``: a ``GBLinear`` and a float64 ``[num_round, 1 + len(evals)]``
    array (the train rmse, then each eval set's, after every round), or for a batch a list of
    ``GBLinear`` and ``[B, num_round, 1 + len(evals)]``."""
    hyper, Bh = _hyper(eta, lambda_, alpha, lambda_bias)         # refused on the host, before any device work
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("gblinear train: chunk must be at least 1")
    import torch

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
    Bq = _batch([yt] + ([ht] if ht else []) + [p for _, ye, he in ev for p in ([ye] + ([he] if he else []))] +
                ([(None, Bh, 0)] if Bh is not None else []))
    B = Bq or 1
    num_round = int(num_round)
    w = torch.zeros(B, F + 1, dtype=torch.float32, device=dev)
    hist = torch.zeros(max(num_round, 1), 1 + len(ev), B, dtype=torch.float64, device=dev)
    hyper_dev = None if Bh is None else torch.from_numpy(hyper).to(dev)
    base = float(np.float32(base_score))
    for c0 in range(0, B, chunk):
        c1 = min(B, c0 + chunk)
        yc, hc, wc = _part(yt, c0, c1), _part(ht, c0, c1), w[c0:c1]
        evc = [(Xe, _part(ye, c0, c1), _part(he, c0, c1), torch.empty(c1 - c0, Xe.n, dtype=torch.float32, device=dev))
               for Xe, ye, he in ev]

        def train_pred(r, pred):
            _rmse(pred, yc, hc, n, c1 - c0, hist[r, 0, c0:c1])

        def after_round(r):
            for k, (Xe, ye, he, ep) in enumerate(evc):
                if Xe.n > 0:
                    _predict_cols(Xe, wc, base, ep)
                    _rmse(ep, ye, he, Xe.n, c1 - c0, hist[r, 1 + k, c0:c1])

        _fit(Xc, yc, hc, hyper if Bh is None else hyper_dev[c0:c1], wc, num_round, base, train_pred, after_round)
    wh = w.cpu().numpy()
    history = hist[:num_round].permute(2, 0, 1).contiguous().cpu().numpy()
    models = [GBLinear(wh[m, :F].reshape(F, 1).copy(), wh[m, F:].copy(), base) for m in range(B)]
    if Bq is None:
        return models[0], history[0]
    return models, history


# -- cross-validation ---------------------------------------------------------------------------
def _grid(grid):
    """A list of (lambda_, alpha) pairs -> float64 [G, 2], checked like ``train``'s arguments."""
    g = np.asarray(list(grid), dtype=np.float64)
    if g.ndim != 2 or g.shape[1] != 2 or g.shape[0] == 0:
        raise ValueError("gblinear cv: grid must be a non-empty list of (lambda_, alpha) pairs")
    _hyper(0.0, g[:, 0], g[:, 1], 0.0)
    return g


def _folds(fold, weight, n, T):
    """Checks of ``cv``'s fold and weight arguments on the host -> (int64 fold [n], K, float32
    weights [T, n]).  Every fold must hold weight for every target, and so must its complement."""
    f = np.asarray(fold)
    if f.shape != (n,) or f.dtype.kind not in "iu":
        raise ValueError(f"gblinear cv: fold must be an integer array of length n = {n}")
    f = f.astype(np.int64)
    if n == 0 or f.min() < 0:
        raise ValueError("gblinear cv: fold values must be 0..K-1 and there must be rows")
    K = int(f.max()) + 1
    if K < 2:
        raise ValueError("gblinear cv: at least two folds are needed")
    wt = np.ones((T, n), np.float32) if weight is None else np.asarray(weight, dtype=np.float32)
    if wt.ndim == 1:
        wt = np.array(np.broadcast_to(wt, (T, n)))
    if wt.shape != (T, n):
        raise ValueError(f"gblinear cv: weight must be [n] or [T, n] with T = {T}, n = {n}")
    if not np.isfinite(wt).all() or (wt < 0).any():
        raise ValueError("gblinear cv: weights must be finite and >= 0")
    for k in range(K):
        rows = f == k
        if not rows.any():
            raise ValueError(f"gblinear cv: fold {k} has no rows")
        for t in range(T):
            if not wt[t, rows].astype(np.float64).sum() > 0:
                raise ValueError(f"gblinear cv: fold {k} has no weight for target {t}")
            if not wt[t, ~rows].astype(np.float64).sum() > 0:
                raise ValueError(f"gblinear cv: the training rows of fold {k} have no weight for target {t}")
    return f, K, wt


def cv_select(heldout, rule="min"):
    """Selection from held-out rmse ``[T, G, K, R]`` in float64 on the host -> ``(score, se, best_g,
    best_round)``.  ``score[t, g, r]``: the mean over the folds, summed in the order k = 0..K-1;
    ``se``: the sample standard deviation over the folds / sqrt(K).  ``rule="min"``: per target the
    (g, r) of least score, ties to the earlier grid entry, then the earlier round.  ``rule="1se"``:
    among the grid entries whose best-round score is <= min + se at the minimum, the earliest, with
    its own best round (order the grid from most to least regularised).  A NaN score (a model that
    diverged) never wins.  ``best_round`` is 1-based."""
    if rule not in ("min", "1se"):
        raise ValueError(f"gblinear cv: rule must be 'min' or '1se', not {rule!r}")
    ho = np.asarray(heldout, dtype=np.float64)
    if ho.ndim != 4 or ho.shape[2] < 2 or 0 in ho.shape:
        raise ValueError("gblinear cv: heldout must be [T, G, K, R] with K >= 2")
    T, G, K, R = ho.shape
    with np.errstate(invalid="ignore"):
        total = ho[:, :, 0].copy()
        for k in range(1, K):
            total = total + ho[:, :, k]
        score = total / K
        ss = np.zeros_like(score)
        for k in range(K):
            d = ho[:, :, k] - score
            ss = ss + d * d
        se = np.sqrt(ss / (K - 1)) / np.sqrt(K)
    rank = np.where(np.isnan(score), np.inf, score)
    best_g, best_round = np.zeros(T, np.int64), np.zeros(T, np.int64)
    for t in range(T):
        if not np.isfinite(rank[t]).any():
            raise RuntimeError(f"gblinear cv: no finite held-out score for target {t}")
        r_of = rank[t].argmin(1)                       # first least round of every grid entry
        best = rank[t, np.arange(G), r_of]
        g = int(best.argmin())                         # first least grid entry
        if rule == "1se":
            g = int(np.nonzero(best <= best[g] + se[t, g, r_of[g]])[0][0])
        best_g[t], best_round[t] = g, r_of[g] + 1
    return score, se, best_g, best_round


@dataclass
class CVResult:
    """What ``cv`` measured and chose.  heldout, train: rmse ``[T, G, K, R]`` after every round, on
    the held-out and on the training rows of fold k; score, se ``[T, G, R]``; best_g ``[T]`` indexes
    ``grid`` (float64 ``[G, 2]``: lambda_, alpha); best_round ``[T]`` is 1-based."""
    heldout: np.ndarray
    train: np.ndarray
    score: np.ndarray
    se: np.ndarray
    best_g: np.ndarray
    best_round: np.ndarray
    grid: np.ndarray
    rule: str = "min"
    eta: float = 0.01
    lambda_bias: float = 0.0
    base_score: float = 2.0
    chunk: int = 256

    def refit(self, X, y, weight=None, evals=(), with_history=False):
        """One model per target on all rows, at its chosen (lambda_, alpha) for ``best_round[t]``
        rounds; targets with the same round count share a launch.  y ``[n]`` or ``[T, n]``, weight
        ``[n]`` or ``[T, n]``, evals as for ``train`` (y_e ``[n_e]`` or ``[T, n_e]``).  Returns the
        ``GBLinear``s in target order, with ``with_history`` also their ``train`` histories
        (``[best_round[t], 1 + len(evals)]`` each)."""
        T = int(self.best_g.shape[0])
        y = np.asarray(y) if not hasattr(y, "dim") else y
        if (y.ndim == 1 and T != 1) or (y.ndim == 2 and y.shape[0] != T):
            raise RuntimeError(f"gblinear refit: y must hold the {T} targets of the cross-validation")
        Xc = X if isinstance(X, ColMatrix) else ColMatrix(X)

        def rows(v, idx):
            return v if v is None or v.ndim == 1 else v[idx]

        def as_array(v):
            return v if v is None or hasattr(v, "dim") else np.asarray(v)

        weight = as_array(weight)
        evals = [(e[0] if isinstance(e[0], ColMatrix) else ColMatrix(e[0], device=Xc.device), as_array(e[1]),
                  as_array(e[2]) if len(e) > 2 else None) for e in evals]
        models, hists = [None] * T, [None] * T
        for R in sorted(set(int(r) for r in self.best_round)):
            idx = np.nonzero(self.best_round == R)[0]
            ms, hs = train(Xc, rows(y, idx), rows(weight, idx), num_round=R, eta=self.eta,
                           lambda_=self.grid[self.best_g[idx], 0], alpha=self.grid[self.best_g[idx], 1],
                           lambda_bias=self.lambda_bias, base_score=self.base_score, chunk=self.chunk,
                           evals=[(Xe, rows(ye, idx), rows(we, idx)) for Xe, ye, we in evals])
            for i, t in enumerate(idx):
                models[t], hists[t] = ms[i], hs[i]
        return (models, hists) if with_history else models


def cv(X, y, fold, grid, *, weight=None, num_round=100, eta=0.01, lambda_bias=0.0, base_score=2.0, rule="min",
       chunk=256):
    """K-fold cross-validation of a grid of penalties, every model of it in one batch over one X.

    y ``[n]`` or ``[T, n]`` (T targets); fold: int ``[n]`` with values 0..K-1; grid: a list of
    ``(lambda_, alpha)`` pairs; weight: base row weights ``[n]`` or ``[T, n]``.  Model (t, g, k)
    trains target t with ``grid[g]`` on the weights ``weight * (fold != k)``: held-out rows stay in
    the matrix at weight zero, and the round kernel's predict pass covers them like any row, so
    the predictions round r+1 starts from give both the train rmse (under ``weight * (fold != k)``)
    and the held-out rmse (under ``weight * (fold == k)``) of round r with no further pass over X.
    The T*G*K models run in launches of at most ``chunk``.  A fold (or its complement) without
    rows or weight for some target is refused before anything is launched.  Selection:
    ``cv_select``.  Returns a ``CVResult``."""
    if rule not in ("min", "1se"):
        raise ValueError(f"gblinear cv: rule must be 'min' or '1se', not {rule!r}")
    g = _grid(grid)
    hp, Bh = _hyper(eta, 0.0, 0.0, lambda_bias)
    if Bh is not None:
        raise ValueError("gblinear cv: eta and lambda_bias are floats (the grid holds lambda_ and alpha)")
    eta, lambda_bias = hp[0], hp[3]
    chunk, num_round = int(chunk), int(num_round)
    if chunk < 1 or num_round < 1:
        raise ValueError("gblinear cv: chunk and num_round must be at least 1")
    Xc_given = isinstance(X, ColMatrix)
    n = X.n if Xc_given else int(X.shape[0])
    yh = y.cpu().numpy() if hasattr(y, "dim") else np.asarray(y)
    if yh.ndim not in (1, 2) or yh.shape[-1] != n:
        raise ValueError(f"gblinear cv: y must be [n] or [T, n] with n = {n}")
    yh = np.atleast_2d(yh).astype(np.float32)
    T, G = yh.shape[0], g.shape[0]
    f, K, wt = _folds(fold, weight.cpu().numpy() if hasattr(weight, "dim") else weight, n, T)

    import torch

    Xc = X if Xc_given else ColMatrix(X)
    dev = Xc.device
    Y, W = torch.from_numpy(yh).to(dev), torch.from_numpy(np.ascontiguousarray(wt)).to(dev)
    fd = torch.from_numpy(f).to(dev)
    B = T * G * K
    m = np.arange(B)
    hyper = np.empty((B, 4))
    hyper[:, 0], hyper[:, 1], hyper[:, 2], hyper[:, 3] = eta, g[(m // K) % G, 0], g[(m // K) % G, 1], lambda_bias
    hyper_dev = torch.from_numpy(hyper).to(dev)
    base = float(np.float32(base_score))
    out = torch.zeros(2, num_round, B, dtype=torch.float64, device=dev)       # train, held-out
    for c0 in range(0, B, chunk):
        c1 = min(B, c0 + chunk)
        b = c1 - c0
        t_of = torch.from_numpy(m[c0:c1] // (G * K)).to(dev)
        held = fd[None, :] == torch.from_numpy(m[c0:c1] % K).to(dev)[:, None]
        yc = (Y[t_of].contiguous(), b, n)
        hc = ((W[t_of] * (~held)).contiguous(), b, n)
        vc = ((W[t_of] * held).contiguous(), b, n)

        def train_pred(r, pred):
            _rmse(pred, yc, hc, n, b, out[0, r, c0:c1])
            _rmse(pred, yc, vc, n, b, out[1, r, c0:c1])

        _fit(Xc, yc, hc, hyper_dev[c0:c1], torch.zeros(b, Xc.F + 1, dtype=torch.float32, device=dev), num_round,
             base, train_pred)
    res = out.permute(0, 2, 1).contiguous().cpu().numpy().reshape(2, T, G, K, num_round)
    score, se, best_g, best_round = cv_select(res[1], rule)
    return CVResult(res[1], res[0], score, se, best_g, best_round, g, rule, eta, lambda_bias, base, chunk)

