"""Host-side mirror of the reference's function surface (lrcn.jl) over the HIP C ABI (include/lrcn.h).

Julia is not available in this image, so the host language above the C ABI is Python; names, argument meaning and
error behaviour follow lrcn.jl so that a test written against the reference reads the same here:

    initweights (lrcn.jl:489)   initstate (:512)   lstm (:528)   lrcn (:540)   loss (:553)   lossgradient (:583)
    initparams / update! (:399, :394)   train1's body -> train_step (:369-394)   average_loss's body -> loss(pdrop=0)
    generate / beam_search (:585-678)   get_convnet -> convnet (:733)   read_image_data's arithmetic (:766-772)

Arrays are torch CUDA tensors holding the reference's COLUMN-MAJOR memory: a Julia R x C matrix is a tensor of
shape (R, C) with strides (1, R) (see `jl_empty`), so `.data_ptr()` is exactly what a Julia `ccall` would pass.
torch is used for device memory, streams and (in dp.py) torch.distributed only -- all arithmetic is in
liblrcn_hip.so.  Token ids are 0-based at this layer (eos=0, bos=1, unk=2).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import BOS, CNNOUT, EOS, LRCN_BF16, LRCN_F32, LRCN_FP8, UNK, LrcnError  # noqa: F401

PARAM_NAMES = ("W1", "b1", "W2", "b2", "Wproj", "Wcnn", "Wembed", "Wout", "bout")
VGG_COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
VGG_MEAN = (123.68, 116.779, 103.939)  # per-channel mean of the VGG-16 averageImage (lrcn.jl:113)


# ------------------------------------------------------------------------------------------------ arrays
def jl_empty(*dims, device="cuda", dtype=torch.float32):
    """Uninitialised tensor of Julia shape `dims` in column-major memory (first index fastest)."""
    t = torch.empty(tuple(reversed(dims)), device=device, dtype=dtype)
    return t.permute(*reversed(range(len(dims))))


def jl_zeros(*dims, device="cuda", dtype=torch.float32):
    t = jl_empty(*dims, device=device, dtype=dtype)
    t.zero_()
    return t


def to_jl(a, device="cuda"):
    """numpy / tensor of logical shape dims -> column-major device tensor of the same logical shape."""
    a = torch.as_tensor(np.asarray(a, dtype=np.float32) if not torch.is_tensor(a) else a)
    out = jl_empty(*a.shape, device=device, dtype=torch.float32)
    out.copy_(a)
    return out


def from_jl(t):
    return t.detach().cpu().numpy()


def _is_jl(t):
    n = t.dim()
    if n == 0 or t.numel() == 0:
        return True
    return t.permute(*reversed(range(n))).is_contiguous()


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise LrcnError("expected a CUDA (HIP) tensor")
    if not _is_jl(t):
        raise LrcnError("tensor is not in the reference's column-major memory order (use to_jl/jl_empty)")
    return C.c_void_p(t.data_ptr())


def _p9(ts):
    if len(ts) != 9:
        raise LrcnError("model must have 9 tensors (lrcn.jl:492)")
    for t in ts:
        if t.dtype != torch.float32:
            raise LrcnError("model tensors must be float32")
    return _lib.P9(*[_ptr(t).value for t in ts])


def param_shapes(E, H1, H2, V, n_layers=2):
    h = (H2 + 1) // 2
    if n_layers == 1:  # LRCN-1f (include/lrcn.h, lrcn_config.n_layers): no W2 / b2 / Wproj
        return [(E + h + H1, 4 * H1), (1, 4 * H1), (0, 0), (0, 0), (0, 0), (CNNOUT, h), (V, E), (H2, V), (1, V)]
    return [(E + H1, 4 * H1), (1, 4 * H1), (H2 + H2, 4 * H2), (1, 4 * H2), (H1, h), (CNNOUT, h), (V, E), (H2, V), (1, V)]


# ------------------------------------------------------------------------------------------------ context
class Context:
    """One lrcn_ctx (one device). Owns scratch only; the caller owns models, gradients, optimizer state."""

    def __init__(self, E, H1, H2, V, max_B, max_T=_lib.MAX_T, lstm_dtype=LRCN_F32, vgg_dtype=LRCN_F32, max_images=0,
                 device=None, n_layers=2):
        if not torch.cuda.is_available():
            raise LrcnError("no MI355X visible: liblrcn_hip has no CPU path")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.E, self.H1, self.H2, self.V = E, H1, H2, V
        self.h = H2 // 2
        self.max_B, self.max_T = max_B, max_T
        self.lstm_dtype, self.vgg_dtype = lstm_dtype, vgg_dtype
        self.n_layers = n_layers
        cfg = _lib.Config(self.device, E, H1, H2, V, max_B, max_T, lstm_dtype, vgg_dtype, max_images, n_layers)
        h = C.c_void_p()
        rc = _lib.lib().lrcn_create(C.byref(cfg), C.byref(h))
        _lib.check(None, rc)
        self._h = h
        self._stream = None
        self.use_stream(torch.cuda.current_stream(self.device))

    def use_stream(self, stream):
        self._stream = stream
        _lib.check(self._h, _lib.lib().lrcn_set_stream(self._h, C.c_void_p(stream.cuda_stream)))

    def sync(self):
        _lib.check(self._h, _lib.lib().lrcn_sync(self._h))

    def set_option(self, option, value):
        """lrcn_set_option: _lib.LRCN_OPT_FUSED_UPDATE / LRCN_OPT_DETERMINISTIC / LRCN_OPT_CONV_CHUNK_BYTES (include/lrcn.h)."""
        self._call("lrcn_set_option", int(option), int(value))

    def params_touched(self):
        """The caller wrote parameter arrays itself (checkpoint load, clipping ...): required under LRCN_OPT_FUSED_UPDATE."""
        self._call("lrcn_params_touched")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().lrcn_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, *args):
        _lib.check(self._h, getattr(_lib.lib(), name)(self._h, *args))


def _dropout(pdrop, seed, mask1, mask2):
    if (pdrop is None or pdrop == 0) and mask1 is None:
        return None, None
    d = _lib.Dropout(float(pdrop or 0.0), int(seed or 0), None, None)
    keep = None
    if mask1 is not None:
        # masks: (T+1, B, E) / (T+1, B, H2) logical arrays; the ABI wants (T+1) column-major blocks (LRCN-1f: mask1 only, (T+1, B, E+h))
        m1 = torch.as_tensor(np.ascontiguousarray(np.transpose(np.asarray(mask1, np.float32), (0, 2, 1)))).cuda()
        d.mask1 = m1.data_ptr()
        keep = [m1]
        if mask2 is not None:
            m2 = torch.as_tensor(np.ascontiguousarray(np.transpose(np.asarray(mask2, np.float32), (0, 2, 1)))).cuda()
            d.mask2 = m2.data_ptr()
            keep.append(m2)
    return d, keep


def _tokens(tokens, device):
    t = torch.as_tensor(np.ascontiguousarray(np.asarray(tokens, dtype=np.int32)) if not torch.is_tensor(tokens) else tokens)
    if t.dim() != 2:
        raise LrcnError("tokens must be [T][B]")
    return t.to(device=device, dtype=torch.int32).contiguous()


def _lens(lens, T, B, norm_tokens):
    """Per-row caption lengths of the variable-length calls (include/lrcn_varlen.h) -> (host int32 array, its ctypes pointer, norm_tokens);
    norm_tokens None = this batch's own count sum(lens + 1)."""
    a = np.ascontiguousarray(np.asarray(lens.cpu() if torch.is_tensor(lens) else lens, dtype=np.int32).reshape(-1))
    if a.shape[0] != B:
        raise LrcnError("lens has %d entries, the batch has %d rows" % (a.shape[0], B))
    n = int(a.astype(np.int64).sum()) + B if norm_tokens is None else int(norm_tokens)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int64(n)


def _row_weights(row_weights, lens, B):
    """Per-row loss weights of the weighted calls (include/lrcn_weighted.h) -> (host float32 array, its ctypes pointer)."""
    if lens is None:
        raise LrcnError("row_weights needs lens (the weighted calls take padded batches; equal lengths: lens[b] = T)")
    a = np.ascontiguousarray(np.asarray(row_weights.detach().cpu() if torch.is_tensor(row_weights) else row_weights, dtype=np.float32).reshape(-1))
    if a.shape[0] != B:
        raise LrcnError("row_weights has %d entries, the batch has %d rows" % (a.shape[0], B))
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


class Sched:
    """Scheduled sampling of one call (include/lrcn_sched.h): a row's eligible input is, with probability eps, a word drawn at `temperature`
    from the row's own logits of the step before; seed keys coins and noise, row0 is the call's first row in the global batch."""
    __slots__ = ("eps", "temperature", "seed", "row0")

    def __init__(self, eps, temperature=1.0, seed=0, row0=0):
        self.eps, self.temperature, self.seed, self.row0 = float(eps), float(temperature), int(seed), int(row0)

    def __iter__(self):
        return iter((self.eps, self.temperature, self.seed, self.row0))


def _sched(sched, B):
    """sched: Sched, (eps, temperature, seed) or (eps, temperature, seed, row0) -> _lib.Sched, checked as the library checks it."""
    t = tuple(sched)
    if len(t) not in (3, 4):
        raise LrcnError("sched must be (eps, temperature, seed[, row0])")
    eps, temp, seed, row0 = float(t[0]), float(t[1]), int(t[2]), int(t[3]) if len(t) == 4 else 0
    if not 0.0 <= eps <= 1.0:   # (a NaN fails every comparison)
        raise LrcnError("sched eps=%r outside [0, 1]" % (t[0],))
    if not 0.0 <= temp < float("inf"):
        raise LrcnError("sched temperature=%r must be finite and >= 0" % (t[1],))
    if not 0 <= seed < 2 ** 64:
        raise LrcnError("sched seed=%r outside [0, 2^64)" % (t[2],))
    if row0 < 0 or row0 + B > 2 ** 32:
        raise LrcnError("sched row0=%d: rows [row0, row0 + %d) must lie in [0, 2^32)" % (row0, B))
    return _lib.Sched(eps, temp, seed, row0)


def _sched_lens(lens, T, B):
    return np.full(B, T, np.int32) if lens is None else lens   # scheduled sampling takes padded batches; equal lengths: lens[b] = T


def sched_stats(ctx):
    """(eligible, drawn) of the most recent scheduled-sampling call: sum(lens) and the coins that fired.  Waits for the context's stream."""
    e, d = C.c_int64(), C.c_int64()
    ctx._call("lrcn_sched_stats", C.byref(e), C.byref(d))
    return int(e.value), int(d.value)


def smooth_stats(ctx):
    """(nll, smoothed) of the most recent call with label_smoothing > 0 (or a direct lrcn_*_smooth call), while no other loss call has
    followed it: the plain negative log-likelihood of the same rows beside the smoothed loss.  Waits for the context's stream."""
    n, s = C.c_double(), C.c_double()
    ctx._call("lrcn_smooth_stats", C.byref(n), C.byref(s))
    return n.value, s.value


def xent_logits(ctx, logits, targets, row_weights=None, B=None, scale=1.0, label_smoothing=0.0, out_dtype=None, want_dlog=True, ld_d=None):
    """The cross-entropy stage alone on the caller's own logits (lrcn_xent_logits): logits a float32 device tensor (M, V), rows stride(0)
    apart; targets int (M) (negative, or >= V: an inactive row); row m belongs to caption m % B (default B = M) and carries
    row_weights[m % B].  -> (dlog, terms, ll_terms): d(logits) (M, V) in out_dtype (torch.float32, the default, or torch.bfloat16; rows
    ld_d apart, default V rounded up to a multiple of 8; None without want_dlog) and the rows' smoothed and plain terms as float64 device
    tensors (M).  Nothing waits for the device."""
    if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1):
        raise LrcnError("logits must be a float32 device tensor (M, V) with contiguous rows")
    M, V = logits.shape
    B = M if B is None else int(B)
    tgt = torch.as_tensor(targets).to(device=logits.device, dtype=torch.int32).contiguous()
    if tgt.numel() != M:
        raise LrcnError("targets has %d entries, logits has %d rows" % (tgt.numel(), M))
    w = None
    if row_weights is not None:
        w = torch.as_tensor(row_weights).to(device=logits.device, dtype=torch.float32).contiguous()
        if w.numel() != B:
            raise LrcnError("row_weights has %d entries, B = %d" % (w.numel(), B))
    out_dtype = out_dtype or torch.float32
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise LrcnError("out_dtype is torch.float32 or torch.bfloat16")
    dlog = None
    if want_dlog:
        ld_d = (V + 7) // 8 * 8 if ld_d is None else int(ld_d)
        dlog = torch.empty((M, ld_d), device=logits.device, dtype=out_dtype)
    terms = torch.empty(M, device=logits.device, dtype=torch.float64)
    ll = torch.empty(M, device=logits.device, dtype=torch.float64)
    ctx._call("lrcn_xent_logits", C.c_void_p(logits.data_ptr()), logits.stride(0), C.c_void_p(tgt.data_ptr()),
              C.c_void_p(w.data_ptr()) if w is not None else None, M, B, V, C.c_float(scale), C.c_float(_smooth(label_smoothing)),
              LRCN_BF16 if out_dtype == torch.bfloat16 else LRCN_F32, C.c_void_p(dlog.data_ptr()) if dlog is not None else None,
              ld_d if dlog is not None else 0, C.c_void_p(terms.data_ptr()), C.c_void_p(ll.data_ptr()))
    return (dlog[:, :V] if dlog is not None else None), terms, ll


# ------------------------------------------------------------------------------------------------ model
def initweights(ctx, seed=42):
    """initweights(atype, hidden, vocab, embed) (lrcn.jl:489-510) -> list of 9 column-major tensors."""
    model = [jl_empty(*s) for s in param_shapes(ctx.E, ctx.H1, ctx.H2, ctx.V, ctx.n_layers)]
    ctx._call("lrcn_init_weights", _p9(model), C.c_uint64(seed))
    return model


def model_from_arrays(arrays):
    """dict name->array or list of 9 arrays (logical reference shapes) -> device model."""
    if isinstance(arrays, dict):
        arrays = [arrays[n] for n in PARAM_NAMES]
    return [to_jl(a) for a in arrays]


def zeros_like_model(model):
    out = []
    for t in model:
        z = jl_empty(*t.shape)
        z.zero_()
        out.append(z)
    return out


def initstate(ctx, batch):
    """initstate(model, batch) (lrcn.jl:512-526): zero (B x H) hidden/cell per layer -- without the reference's
    spurious third layer and without aliasing all entries to one array."""
    if ctx.n_layers == 1:
        return [jl_zeros(batch, ctx.H1), jl_zeros(batch, ctx.H1)]
    return [jl_zeros(batch, ctx.H1), jl_zeros(batch, ctx.H1), jl_zeros(batch, ctx.H2), jl_zeros(batch, ctx.H2)]


def lstm(ctx, weight, bias, hidden, cell, input):
    """lstm(weight,bias,hidden,cell,input) (lrcn.jl:528-538) -> (hidden, cell)."""
    B, X = input.shape
    H = hidden.shape[1]
    h_out, c_out = jl_empty(B, H), jl_empty(B, H)
    ctx._call("lrcn_lstm", _ptr(weight), _ptr(bias), X, H, B, _ptr(input), _ptr(hidden), _ptr(cell), _ptr(h_out), _ptr(c_out))
    return h_out, c_out


def lrcn(ctx, w, s, x_cnn, x_lstm, mask1=None, mask2=None):
    """lrcn(w, s, x_cnn, x_lstm; pdrop) (lrcn.jl:540-551): one timestep; mutates s like the reference; returns logits.
    Dropout enters as explicit multiplier arrays (B x E, B x H2) so a step is reproducible."""
    B = x_lstm.shape[0]
    logits = jl_empty(B, ctx.V)
    st = _lib.P4(*([_ptr(t).value for t in s] + [None] * (4 - len(s))))
    ctx._call("lrcn_step", _p9(w), st, B, _ptr(x_cnn), _ptr(x_lstm), _ptr(mask1), _ptr(mask2), _ptr(logits))
    return logits


def _smooth(label_smoothing):
    """label_smoothing -> float in [0, 1], checked as the library checks it (a NaN fails every comparison)."""
    eps = float(label_smoothing or 0.0)
    if not 0.0 <= eps <= 1.0:
        raise LrcnError("label_smoothing=%r outside [0, 1]" % (label_smoothing,))
    return eps


def _caption_call(ctx, param, feats, tokens, norm_B, drop, lens, norm_tokens, row_weights, sched, want_loss=True, grads=None, optim=None,
                  gclip=0.0, return_fed=False, return_logits=False, label_smoothing=0.0):
    """The one path of loss / lossgradient / train_step (optim given) to the library -> (loss or None, fed, logits).  The entry point is named
    by the first of label_smoothing > 0, sched, row_weights, lens that is given: lrcn_{loss, loss_grad, train_step}{_smooth, _sched, _w, _var,
    ""}, and a step with none of the first three takes max_norm (gclip) only as lrcn_train_step[_var]_clip.  The _smooth entries take
    row_weights and sched as options; without lens their rows are equal-length captions: lens[b] = T, norm_tokens = (norm_B or B) (T + 1).
    Every check runs before optim.t moves."""
    tok = _tokens(tokens, feats.device)
    T, B = tok.shape
    ss = _sched(sched, B) if sched is not None else None
    eps = _smooth(label_smoothing)
    if ss is None and (return_fed or return_logits):
        raise LrcnError("return_fed / return_logits need sched")
    if eps > 0 and return_logits:
        raise LrcnError("return_logits is not available with label_smoothing (include/lrcn_smooth.h has no logits_out)")
    if eps > 0 and lens is None and norm_tokens is None:
        norm_tokens = (norm_B or B) * (T + 1)   # the equal-length normaliser
    if ss is not None or eps > 0:
        lens = _sched_lens(lens, T, B)
    wa = _row_weights(row_weights, lens, B) if row_weights is not None else None
    la = _lens(lens, T, B, norm_tokens) if lens is not None else None
    d, keep = _dropout(*drop)
    form = "_smooth" if eps > 0 else "_sched" if ss is not None else "_w" if wa is not None else "_var" if la is not None else ""
    name = ("lrcn_train_step" if optim is not None else "lrcn_loss_grad" if grads is not None else "lrcn_loss") + form
    args = [_p9(param)] + ([_p9(grads), _p9(optim.m), _p9(optim.v)] if optim is not None else []) + [_ptr(feats), C.c_void_p(tok.data_ptr())]
    if la is not None:
        args.append(la[1])
    if form in ("_smooth", "_sched", "_w"):
        args.append(wa[1] if wa else None)
    args += [T, B, la[2] if la is not None else norm_B or B, C.byref(d) if d else None]
    if ss is not None or form == "_smooth":
        args.append(C.byref(ss) if ss is not None else None)
    fed = torch.empty((T + 1, B), device=feats.device, dtype=torch.int32) if return_fed else None
    logits = torch.empty((T + 1, ctx.V, B), device=feats.device, dtype=torch.float32) if return_logits else None  # blocks of B x V column-major
    if optim is not None:
        optim.t += 1
        args += ([C.c_float(eps)] if form == "_smooth" else []) + [optim.t, optim.lr, optim.beta1, optim.beta2, optim.eps]
        if form in ("_smooth", "_sched", "_w"):   # these three always take max_norm, the others only as their _clip namesakes
            args.append(gclip)
        elif gclip > 0:
            name += "_clip"
            args.append(gclip)
    elif form == "_smooth":
        args += [C.c_void_p(fed.data_ptr()) if return_fed else None, C.c_float(eps)] + ([_p9(grads)] if grads is not None else [])
    else:
        args += [_p9(grads)] if grads is not None else []
        if ss is not None:
            args += [C.c_void_p(fed.data_ptr()) if return_fed else None, C.c_void_p(logits.data_ptr()) if return_logits else None]
    out = C.c_double()
    ctx._call(name, *args, C.byref(out) if want_loss else None)
    del keep, la, wa   # the host arrays and masks the arguments point into: held until the call has returned
    return (out.value if want_loss else None), fed, logits


def loss(ctx, param, feats, tokens, norm_B=None, pdrop=0.0, seed=0, mask1=None, mask2=None, lens=None, norm_tokens=None, row_weights=None,
         sched=None, label_smoothing=0.0):
    """loss(param,state,input,sequence,range; pdrop) (lrcn.jl:553-581).  feats: B x 4096 (column-major);
    tokens: [T][B] = sequence[range]; norm_B = the reference's global `batchsize` (default B).
    lens (int [B], 0 <= lens[b] <= T): the padded batch of include/lrcn_varlen.h -- row b counts lens[b] + 1 terms, the sum is divided by
    norm_tokens (default: this batch's sum(lens + 1); data parallelism: the global batch's) and norm_B is not used.
    row_weights (float [B], with lens): row b's terms are multiplied by row_weights[b], of either sign or 0 (include/lrcn_weighted.h).
    sched (Sched, or (eps, temperature, seed[, row0])): scheduled sampling (include/lrcn_sched.h); lens then defaults to [T] * B.
    label_smoothing (0 <= eps <= 1; include/lrcn_smooth.h): every active row is scored against (1 - eps) onehot + eps / V, inside the loss
    kernels, and the value returned is the smoothed loss (smooth_stats() has the plain one).  It combines with lens, row_weights and sched;
    without lens the normaliser stays the equal-length one, norm_B (T + 1).  0 is the call without the keyword."""
    return _caption_call(ctx, param, feats, tokens, norm_B, (pdrop, seed, mask1, mask2), lens, norm_tokens, row_weights, sched,
                         label_smoothing=label_smoothing)[0]


def lossgradient(ctx, param, feats, tokens, norm_B=None, pdrop=0.0, seed=0, mask1=None, mask2=None, grads=None,
                 want_loss=True, lens=None, norm_tokens=None, row_weights=None, sched=None, return_fed=False, return_logits=False,
                 label_smoothing=0.0):
    """lossgradient = grad(loss) (lrcn.jl:583) -> (grads, loss).  `grads` may be a preallocated 9-list.  lens / norm_tokens / row_weights /
    sched / label_smoothing: as loss().  With sched, return_fed / return_logits append the words that were fed ((T+1, B) int32 numpy) and the logits the
    draws were made from ((T+1, B, V) float32 numpy) to the result."""
    if grads is None:
        grads = [jl_empty(*t.shape) for t in param]
    val, fed, logits = _caption_call(ctx, param, feats, tokens, norm_B, (pdrop, seed, mask1, mask2), lens, norm_tokens, row_weights, sched,
                                     want_loss, grads, return_fed=return_fed, return_logits=return_logits, label_smoothing=label_smoothing)
    res = (grads, val)
    if return_fed:
        res += (fed.cpu().numpy(),)
    if return_logits:
        res += (logits.permute(0, 2, 1).cpu().numpy(),)
    return res


def last_loss(ctx):
    out = C.c_double()
    ctx._call("lrcn_last_loss", C.byref(out))
    return out.value


def forward_logits(ctx, param, feats, tokens):
    """Per-step logits of the loss forward pass: (T+1, B, V) numpy (parity probe)."""
    tok = _tokens(tokens, feats.device)
    T, B = tok.shape
    out = torch.empty((T + 1, ctx.V, B), device=feats.device, dtype=torch.float32)  # blocks of B x V column-major
    ctx._call("lrcn_forward_logits", _p9(param), _ptr(feats), C.c_void_p(tok.data_ptr()), T, B, C.c_void_p(out.data_ptr()))
    return out.permute(0, 2, 1).cpu().numpy()


class Adam:
    """One Knet Adam() per tensor (initparams, lrcn.jl:399-405) with Knet's defaults."""

    def __init__(self, model, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
        self.lr, self.beta1, self.beta2, self.eps = lr, beta1, beta2, eps
        self.t = 0
        self.m = zeros_like_model(model)
        self.v = zeros_like_model(model)


def initparams(model):
    return Adam(model)


def _stream_arg(stream):
    return C.c_void_p(stream.cuda_stream) if stream is not None else None


def grad_sumsq(ctx, g, slot=0, stream=None, group=-1):
    """Sum of squares (a double in the context's control block, include/lrcn_clip.h) of a gradient, on `stream`: g a float32 tensor ->
    slot `slot`; g a model's nine gradients -> tensor k into slot k, for the tensors of gradient group `group` (-1: all nine)."""
    if torch.is_tensor(g):
        assert g.dtype == torch.float32 and g.is_contiguous()
        ctx._call("lrcn_grad_sumsq", C.c_void_p(g.data_ptr()) if g.numel() else None, g.numel(), int(slot), _stream_arg(stream))
    else:
        ctx._call("lrcn_grad_sumsq_model", _p9(g), int(group), _stream_arg(stream))


def clip_slots(ctx, n_slots=9):
    """The control block's first n_slots sums of squares as a float64 device tensor that aliases them (a sharded job all-reduces it)."""
    p = C.c_void_p()
    ctx._call("lrcn_clip_slots", C.byref(p))

    class _Mem:   # the CUDA array interface: a view, the context keeps the memory
        __cuda_array_interface__ = {"shape": (int(n_slots),), "typestr": "<f8", "data": (p.value, False), "version": 2}
    return torch.as_tensor(_Mem(), device=torch.device("cuda", ctx.device))


def clip_set(ctx, max_norm, n_slots=9, stream=None):
    """norm = sqrt(slot[0] + ... + slot[n_slots - 1]), skip = not finite, scale = max_norm / norm when norm > max_norm (lrcn_clip_set)."""
    ctx._call("lrcn_clip_set", int(n_slots), float(max_norm), _stream_arg(stream))


def clip_stats(ctx):
    """Waits for the context's stream: {last_norm, last_scale, last_skipped, steps, clipped, skipped} (lrcn_clip_stats)."""
    st = _lib.ClipStats()
    ctx._call("lrcn_clip_stats", C.byref(st))
    return {"last_norm": st.last_norm, "last_scale": st.last_scale, "last_skipped": int(st.last_skipped), "steps": int(st.steps),
            "clipped": int(st.clipped), "skipped": int(st.skipped)}


def update(ctx, param, grads, optim, clipped=False):
    """update!(param, gloss, optim) (lrcn.jl:394).  clipped: on grads * scale, scale and skip read from the context's control block."""
    optim.t += 1
    ctx._call("lrcn_adam_update_clipped" if clipped else "lrcn_adam_update", _p9(param), _p9(grads), _p9(optim.m), _p9(optim.v), optim.t, optim.lr, optim.beta1,
              optim.beta2, optim.eps)


def update_group(ctx, param, grads, optim, group, stream=None, clipped=False):
    """update! for the tensors of one gradient group (include/lrcn.h lrcn_adam_update_group) on `stream`; the caller
    advances optim.t once per step, before the first group."""
    ctx._call("lrcn_adam_update_group_clipped" if clipped else "lrcn_adam_update_group", _p9(param), _p9(grads), _p9(optim.m), _p9(optim.v), int(group), optim.t, optim.lr,
              optim.beta1, optim.beta2, optim.eps, C.c_void_p(stream.cuda_stream) if stream is not None else None)


def update_flat(ctx, w, g, m, v, optim, stream=None, clipped=False):
    """The Adam arithmetic on one flat run of floats (lrcn_adam_update_flat): w, g, m, v are 1-D float32 tensors of equal length; the
    caller advances optim.t once per step."""
    n = w.numel()
    assert g.numel() == n and m.numel() == n and v.numel() == n
    ctx._call("lrcn_adam_update_flat_clipped" if clipped else "lrcn_adam_update_flat", C.c_void_p(w.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(m.data_ptr()), C.c_void_p(v.data_ptr()),
              n, optim.t, optim.lr, optim.beta1, optim.beta2, optim.eps, C.c_void_p(stream.cuda_stream) if stream is not None else None)


def refresh_shadows_group(ctx, param, group, stream=None):
    """lrcn_refresh_shadows_group: the next step's shadow weights of one gradient group, on `stream`, from the parameters as they are now."""
    ctx._call("lrcn_refresh_shadows_group", _p9(param), int(group), C.c_void_p(stream.cuda_stream) if stream is not None else None)


def train_step(ctx, param, optim, grads, feats, tokens, norm_B=None, pdrop=0.4, seed=0, want_loss=False, lens=None, norm_tokens=None,
               gclip=0.0, row_weights=None, sched=None, label_smoothing=0.0):
    """Body of train1's batch loop (lrcn.jl:369-394): lossgradient + update!, one C call.  lens / norm_tokens / row_weights / sched /
    label_smoothing: as loss().
    gclip > 0: the global gradient norm is clipped to it on the device (include/lrcn_clip.h; clip_stats() has the counters)."""
    return _caption_call(ctx, param, feats, tokens, norm_B, (pdrop, seed, None, None), lens, norm_tokens, row_weights, sched, want_loss, grads,
                         optim, float(gclip or 0.0), label_smoothing=label_smoothing)[0]


def comm_unique_id():
    """RCCL unique id (bytes) for lrcn_comm_init: rank 0 creates it, the host program distributes it."""
    buf = (C.c_char * 128)()
    _lib.check(None, _lib.lib().lrcn_comm_unique_id(buf))
    return bytes(buf)


def comm_probe(ctx):
    """LOCAL check that comm_init can be entered on this rank (librccl loadable, symbols resolved, no communicator yet): lrcn_comm_probe.
    -> (ok, message)"""
    try:
        ctx._call("lrcn_comm_probe")
        return True, ""
    except LrcnError as e:
        return False, str(e)


def comm_init(ctx, world, rank, unique_id):
    """Bind ctx to rank `rank` of a `world`-rank RCCL communicator (collective over the ranks): lrcn_comm_init."""
    buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
    ctx._call("lrcn_comm_init", int(world), int(rank), buf)


def set_embed_rows_buffer(ctx, rows, tok):
    """Sparse exchange of the embedding gradient (lrcn_set_embed_rows_buffer): lossgradient writes its (T+1) B rows of d(x_lstm) and their token
    ids into `rows` (float32, capacity x E) / `tok` (int32, capacity) instead of the dense gradient of Wembed; (None, None) turns it off."""
    if rows is None:
        ctx._call("lrcn_set_embed_rows_buffer", None, None, 0)
    else:
        ctx._call("lrcn_set_embed_rows_buffer", C.c_void_p(rows.data_ptr()), C.c_void_p(tok.data_ptr()), int(tok.numel()))


def embed_grad_from_rows(ctx, rows, tok, n_rows, grad_wembed, stream=None):
    """The dense d Wembed (V x E column-major) from the rows of ALL ranks, summed per token in one fixed order (lrcn_embed_grad_from_rows)."""
    ctx._call("lrcn_embed_grad_from_rows", C.c_void_p(rows.data_ptr()), C.c_void_p(tok.data_ptr()), int(n_rows), _ptr(grad_wembed),
              C.c_void_p(stream.cuda_stream) if stream is not None else None)


def comm_set_stream(ctx, stream):
    """The stream for the context's collectives and per-group updates (lrcn_comm_set_stream); the caller keeps `stream` alive."""
    ctx._call("lrcn_comm_set_stream", C.c_void_p(stream.cuda_stream))


def comm_destroy(ctx):
    ctx._call("lrcn_comm_destroy")


def allreduce_grads(ctx, grads, group=-1):
    """lrcn_allreduce_grads: in-place all-reduce(SUM) of one gradient group (or all) on the context's group stream."""
    ctx._call("lrcn_allreduce_grads", _p9(grads), int(group))


def comm_join(ctx):
    ctx._call("lrcn_comm_join")


def train_step_dp(ctx, param, optim, grads, feats, tokens, norm_B=None, pdrop=0.4, seed=0, img_u8=None, mean=VGG_MEAN, normalize=False,
                  want_loss=False):
    """The data-parallel step in one C call (lrcn_train_step_dp): [VGG forward of img_u8 into feats] + lossgradient + per-group
    all-reduce over the ranks + per-group Adam.  feats: B x 4096 column-major (input, or output buffer when img_u8 is given)."""
    tok = _tokens(tokens, feats.device)
    T, B = tok.shape
    d, keep = _dropout(pdrop, seed, None, None)
    optim.t += 1
    out = C.c_double()
    m = (C.c_float * 3)(*mean) if mean is not None else None
    ctx._call("lrcn_train_step_dp", _p9(param), _p9(grads), _p9(optim.m), _p9(optim.v),
              C.c_void_p(img_u8.data_ptr()) if img_u8 is not None else None, m, int(bool(normalize)), _ptr(feats), C.c_void_p(tok.data_ptr()),
              T, B, norm_B or B, C.byref(d) if d else None, optim.t, optim.lr, optim.beta1, optim.beta2, optim.eps,
              C.byref(out) if want_loss else None)
    del keep
    return out.value if want_loss else None


def average_loss(ctx, param, batches):
    """average_loss (lrcn.jl:407-486): forward-only NLL over batches [(feats, tokens), ...], pdrop 0, captions longer
    than 28 tokens skipped (:438); returns -total/count with count = sum of B*(T+1)."""
    total, count = 0.0, 0
    for feats, tokens in batches:
        T, B = np.asarray(tokens).shape if not torch.is_tensor(tokens) else tokens.shape
        if T > 28:
            continue
        n = B * (T + 1)
        total += avg_loss_batch(ctx, param, feats, tokens) * n
        count += n
    return total / max(count, 1)


def avg_loss_batch(ctx, param, feats, tokens, lens=None):
    """The body of average_loss's batch loop (lrcn.jl:452-475): pdrop 0, the loss divided by the batch's own size (lrcn_avg_loss_batch).
    lens: the padded batch of include/lrcn_varlen.h, divided by its own token count sum(lens + 1)."""
    if lens is not None:
        return loss(ctx, param, feats, tokens, lens=lens)
    tok = _tokens(tokens, feats.device)
    T, B = tok.shape
    out = C.c_double()
    ctx._call("lrcn_avg_loss_batch", _p9(param), _ptr(feats), C.c_void_p(tok.data_ptr()), T, B, C.byref(out))
    return out.value


def profile(ctx, level):
    """lrcn_profile: 0 off, 1 the convolution launches of every VGG forward, 2 also the HBM-bound segments (lrcn_profile_segment)."""
    ctx._call("lrcn_profile", int(level))


def profile_segments(ctx):
    """-> {segment: (milliseconds, brackets, algorithmic bytes)} accumulated since profile(ctx, 2) (synchronises the device)."""
    out = {}
    for i, name in enumerate(_lib.SEGMENTS):
        ms, n, by = C.c_double(), C.c_int64(), C.c_double()
        ctx._call("lrcn_profile_segment", i, C.byref(ms), C.byref(n), C.byref(by))
        out[name] = (ms.value, n.value, by.value)
    return out


def beam_search(ctx, param, feat, beam_width, nword):
    """generate's decode (lrcn.jl:609-633) + beam_search (:644-678) -> (token ids incl. bos, probability)."""
    out = (C.c_int32 * (nword + 3))()
    n = C.c_int()
    p = C.c_float()
    ctx._call("lrcn_beam_search", _p9(param), _ptr(feat), beam_width, nword, out, C.byref(n), C.byref(p))
    return list(out[:n.value]), p.value


def beam_search_batch(ctx, param, feats, beam_width, nword):
    """beam_search for N images in one device-resident decode (lrcn_beam_search_batch): feats N x 4096 ->
    [(token ids incl. bos, probability)] per image; N * beam_width <= max_B."""
    N = feats.shape[0]
    L = nword + 2
    out = (C.c_int32 * (N * L))()
    n = (C.c_int * N)()
    p = (C.c_float * N)()
    ctx._call("lrcn_beam_search_batch", _p9(param), _ptr(feats), N, beam_width, nword, out, n, p)
    return [(list(out[i * L:i * L + n[i]]), p[i]) for i in range(N)]


def sample_batch(ctx, param, feats, nsamples, nword, temperature=1.0, top_k=0, seed=0, top_p=1.0, return_counts=False):
    """Sampled generation for N images in one device-resident decode (lrcn_sample_batch, include/lrcn_sample.h; the sample() path of
    lrcn.jl:613-621, 680-687): feats N x 4096 -> per image nsamples x (token ids incl. bos, log-likelihood); N * nsamples <= max_B.
    temperature 0 = greedy (beam width 1); top_k 0 = the whole vocabulary.  The draws of image i depend only on (seed, i, sample, step).
    top_p < 1 (nucleus sampling: the most probable words that together hold that share of the mass, after the top_k cut) or top_k > 32 go
    through lrcn_sample_batch_p (include/lrcn_nucleus.h), as does return_counts: then the result is (that list, counts) with counts a numpy
    [N][nsamples][nword + 1] array of the admitted set's size at every step (0 after a row's end)."""
    N, S, L = feats.shape[0], nsamples, nword + 2
    out = (C.c_int32 * (N * S * L))()
    n = (C.c_int * (N * S))()
    lp = (C.c_float * (N * S))()
    cnt = None
    if top_p < 1.0 or top_k > 32 or return_counts or top_p != top_p:
        cnt = np.zeros((N, S, nword + 1), np.int32) if return_counts else None
        ctx._call("lrcn_sample_batch_p", _p9(param), _ptr(feats), N, S, nword, float(temperature), int(top_k), float(top_p),
                  int(seed) & 0xFFFFFFFFFFFFFFFF, out, n, lp, cnt.ctypes.data_as(C.POINTER(C.c_int32)) if return_counts else None)
    else:
        ctx._call("lrcn_sample_batch", _p9(param), _ptr(feats), N, S, nword, float(temperature), int(top_k), int(seed) & 0xFFFFFFFFFFFFFFFF, out, n, lp)
    res = [[(list(out[r * L:r * L + n[r]]), lp[r]) for r in range(i * S, (i + 1) * S)] for i in range(N)]
    return (res, cnt) if return_counts else res


def sample_logits(ctx, logits, S, current, temperature=1.0, top_k=0, top_p=1.0, seed=0):
    """One step of the sampler's selection and draw on the caller's own logits (lrcn_sample_logits, include/lrcn_nucleus.h): logits numpy
    [R][V] f32, row r = image r // S, sample r % S, step `current` of the noise counter -> numpy (tokens [R] int32, log softmax(z)[token] [R]
    f32, admitted-set sizes [R] int32).  Independent of the context's model sizes."""
    z = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).to("cuda:%d" % ctx.device)
    R, V = z.shape
    tok = torch.empty(R, dtype=torch.int32, device=z.device)
    lp = torch.empty(R, dtype=torch.float32, device=z.device)
    cnt = torch.empty(R, dtype=torch.int32, device=z.device)
    torch.cuda.synchronize(z.device)   # the upload has landed whichever stream the context runs on
    ctx._call("lrcn_sample_logits", C.c_void_p(z.data_ptr()), V, R, V, int(S), int(current), float(temperature), int(top_k), float(top_p),
              int(seed) & 0xFFFFFFFFFFFFFFFF, C.c_void_p(tok.data_ptr()), C.c_void_p(lp.data_ptr()), C.c_void_p(cnt.data_ptr()))
    ctx.sync()
    return tok.cpu().numpy(), lp.cpu().numpy(), cnt.cpu().numpy()


def beam_nbest_batch(ctx, param, feats, beam_width, nword, alpha=0.0):
    """n-best beam search for N images in one device-resident decode (lrcn_beam_nbest_batch, include/lrcn_nbest.h): log space, a pool of
    finished hypotheses, length normalisation score = logp / len^alpha (len = tokens after bos) and an exact early stop.  feats N x 4096 ->
    per image up to beam_width (token ids incl. bos, logp, score), best score first; N * beam_width <= max_B."""
    N, K, L = feats.shape[0], beam_width, nword + 2
    out = (C.c_int32 * (N * K * L))()
    n = (C.c_int * (N * K))()
    lp = (C.c_float * (N * K))()
    sc = (C.c_float * (N * K))()
    ctx._call("lrcn_beam_nbest_batch", _p9(param), _ptr(feats), N, K, nword, float(alpha), out, n, lp, sc)
    toks = np.ctypeslib.as_array(out).reshape(N * K, L).tolist()   # (one conversion: N * K rows of ctypes slices cost milliseconds)
    n, lp, sc = list(n), list(lp), list(sc)
    return [[(toks[r][:n[r]], lp[r], sc[r]) for r in range(i * K, (i + 1) * K) if n[r] > 0] for i in range(N)]


def nbest_captions(ctx, param, feats, index_to_word, beam_width, nword, alpha=0.0, normalize=False):
    """beam_nbest_batch as caption text: per image the list of (caption, logp, score), best score first."""
    if normalize:
        f = from_jl(feats)
        feats = to_jl(f / f.sum(axis=1, keepdims=True))  # input/sum(input) per image (lrcn.jl:597)
    return [[(_caption(toks, index_to_word), lp, sc) for toks, lp, sc in entries]
            for entries in beam_nbest_batch(ctx, param, feats, beam_width, nword, alpha)]


def beam_diverse_batch(ctx, param, feats, beam_width, groups, strength, nword, alpha=0.0):
    """Diverse beam search for N images in one device-resident decode (lrcn_beam_diverse_batch, include/lrcn_diverse.h): beam_width beams in
    `groups` groups of beam_width / groups, each an n-best beam whose proposals lose `strength` per live slot that an earlier group of the
    image filled with the same word at the same step.  logp is the model's log-likelihood of the caption (the penalty never enters it).
    feats N x 4096 -> per image a list of `groups` lists of (token ids incl. bos, logp, score), each best score first."""
    N, K, G, L = feats.shape[0], beam_width, groups, nword + 2
    out = (C.c_int32 * (N * K * L))()
    n = (C.c_int * (N * K))()
    lp = (C.c_float * (N * K))()
    sc = (C.c_float * (N * K))()
    ctx._call("lrcn_beam_diverse_batch", _p9(param), _ptr(feats), N, K, G, float(strength), nword, float(alpha), out, n, lp, sc)
    toks = np.ctypeslib.as_array(out).reshape(N * K, L).tolist()
    n, lp, sc = list(n), list(lp), list(sc)
    Kp = K // G
    return [[[(toks[r][:n[r]], lp[r], sc[r]) for r in range(i * K + g * Kp, i * K + (g + 1) * Kp) if n[r] > 0] for g in range(G)] for i in range(N)]


def diverse_captions(ctx, param, feats, index_to_word, beam_width, groups, strength, nword, alpha=0.0, normalize=False):
    """beam_diverse_batch as caption text: per image the list of groups, each a list of (caption, logp, score), best score first."""
    if normalize:
        f = from_jl(feats)
        feats = to_jl(f / f.sum(axis=1, keepdims=True))  # input/sum(input) per image (lrcn.jl:597)
    return [[[(_caption(toks, index_to_word), lp, sc) for toks, lp, sc in grp] for grp in img]
            for img in beam_diverse_batch(ctx, param, feats, beam_width, groups, strength, nword, alpha)]


def _constraints(banned, min_len, no_repeat_ngram):
    """-> (lrcn_constraints, the array its list points to, which the caller keeps alive over the call)"""
    ids = [int(v) for v in banned]
    arr = (C.c_int32 * max(len(ids), 1))(*ids)
    return _lib.Constraints(arr if ids else None, len(ids), int(min_len), int(no_repeat_ngram)), arr


def beam_constrained_batch(ctx, param, feats, beam_width, nword, alpha=0.0, banned=(), min_len=0, no_repeat_ngram=0, groups=0, strength=0.0):
    """Constrained beam search (lrcn_beam_constrained_batch, include/lrcn_constrain.h): the n-best beam (groups 0) or diverse beam search
    (groups >= 1, with `strength`) that never proposes a word of `banned` (token ids in [1, V); not eos), never ends a caption in eos
    before it has min_len words, and with no_repeat_ngram = n >= 1 never completes an n-gram the caption already holds.  logp stays the
    model's log-likelihood of the caption (the bans do not renormalise).  Returns what beam_nbest_batch returns for groups == 0 and what
    beam_diverse_batch returns for groups >= 1; with nothing constrained it is that call, bit for bit."""
    N, K, G, L = feats.shape[0], beam_width, int(groups), nword + 2
    out = (C.c_int32 * (N * K * L))()
    n = (C.c_int * (N * K))()
    lp = (C.c_float * (N * K))()
    sc = (C.c_float * (N * K))()
    cons, keep = _constraints(banned, min_len, no_repeat_ngram)
    ctx._call("lrcn_beam_constrained_batch", _p9(param), _ptr(feats), N, K, G, float(strength), nword, float(alpha), C.byref(cons), out, n, lp, sc)
    del keep
    toks = np.ctypeslib.as_array(out).reshape(N * K, L).tolist()
    n, lp, sc = list(n), list(lp), list(sc)
    if G == 0:
        return [[(toks[r][:n[r]], lp[r], sc[r]) for r in range(i * K, (i + 1) * K) if n[r] > 0] for i in range(N)]
    Kp = K // G
    return [[[(toks[r][:n[r]], lp[r], sc[r]) for r in range(i * K + g * Kp, i * K + (g + 1) * Kp) if n[r] > 0] for g in range(G)] for i in range(N)]


def constrained_captions(ctx, param, feats, index_to_word, beam_width, nword, alpha=0.0, banned=(), min_len=0, no_repeat_ngram=0, groups=0,
                         strength=0.0, normalize=False):
    """beam_constrained_batch as caption text: as nbest_captions (groups == 0) or diverse_captions (groups >= 1)."""
    if normalize:
        f = from_jl(feats)
        feats = to_jl(f / f.sum(axis=1, keepdims=True))  # input/sum(input) per image (lrcn.jl:597)
    res = beam_constrained_batch(ctx, param, feats, beam_width, nword, alpha, banned, min_len, no_repeat_ngram, groups, strength)
    if groups == 0:
        return [[(_caption(toks, index_to_word), lp, sc) for toks, lp, sc in entries] for entries in res]
    return [[[(_caption(toks, index_to_word), lp, sc) for toks, lp, sc in grp] for grp in img] for img in res]


def constrained_topk_logits(ctx, logits, K, hist, current, banned=(), min_len=0, no_repeat_ngram=0):
    """One step of the constrained top-K on the caller's own logits (lrcn_constrained_topk_logits, include/lrcn_constrain.h): logits numpy
    [R][V] f32 (V % 4 == 0, or a torch device tensor whose row stride is a multiple of 4 and >= V = its column count), hist numpy [R][>=
    current] int32 with bos at position 0 -> numpy (columns [R][K] int32, logp [R][K] f32).  Independent of the context's model sizes."""
    dev = "cuda:%d" % ctx.device
    if isinstance(logits, torch.Tensor):
        z = logits
    else:
        a = np.ascontiguousarray(logits, dtype=np.float32)
        ld = (a.shape[1] + 3) // 4 * 4   # rows 16 bytes apart
        z = torch.zeros((a.shape[0], ld), dtype=torch.float32, device=dev)[:, :a.shape[1]]
        z.copy_(torch.from_numpy(a))
    R, V = z.shape
    h = torch.from_numpy(np.ascontiguousarray(hist, dtype=np.int32)).to(dev)
    idx = torch.empty((R, K), dtype=torch.int32, device=z.device)
    lp = torch.empty((R, K), dtype=torch.float32, device=z.device)
    cons, keep = _constraints(banned, min_len, no_repeat_ngram)
    torch.cuda.synchronize(z.device)   # the uploads have landed whichever stream the context runs on
    ctx._call("lrcn_constrained_topk_logits", C.c_void_p(z.data_ptr()), z.stride(0), R, V, int(K), C.byref(cons), C.c_void_p(h.data_ptr()),
              h.shape[1], int(current), C.c_void_p(idx.data_ptr()), C.c_void_p(lp.data_ptr()))
    del keep
    ctx.sync()
    return idx.cpu().numpy(), lp.cpu().numpy()


def _forced(forced, N):
    """forced: one list of sets (each a list of alternative token ids) for all N images, or a list of N such lists (None or [] for an
    image: no sets).  -> (lrcn_forced or None, the array it points to, the N lists of sets)"""
    forced = list(forced) if forced is not None else []
    first = next((f for f in forced if f is not None and len(f)), None)   # a set (its first entry an id) or an image's list of sets
    if first is None or np.isscalar(first[0]):
        forced = [[f for f in forced if f is not None and len(f)]] * N   # one list of sets for every image
    elif len(forced) != N:
        raise LrcnError("forced words: %d lists of sets for %d images" % (len(forced), N))
    sets = [[[int(v) for v in alt] for alt in (img or [])] for img in forced]
    Cn = max([len(img) for img in sets] + [0])
    An = max([len(alt) for img in sets for alt in img] + [1])
    if Cn == 0:
        return None, None, sets
    arr = (C.c_int32 * (N * Cn * An))(*([-1] * (N * Cn * An)))
    for n, img in enumerate(sets):
        for c, alt in enumerate(img):
            for a, v in enumerate(alt):
                arr[(n * Cn + c) * An + a] = v
    return _lib.Forced(arr, Cn, An), arr, sets


def meets(tokens, sets):
    """Does a caption (token ids) hold a word of every non-empty set of `sets` (a list of lists of alternative ids)?"""
    have = set(int(t) for t in tokens)
    return all(any(int(v) in have for v in alt) for alt in sets if len(alt))


def beam_forced_batch(ctx, param, feats, beam_width, nword, alpha=0.0, forced=(), banned=(), min_len=0, no_repeat_ngram=0):
    """Forced-word beam search (lrcn_beam_forced_batch, include/lrcn_forced.h): the n-best beam under the constraints of
    beam_constrained_batch whose every returned caption holds a word of each of its image's sets.  forced: one list of sets for all
    images -- [[dog, dogs], [frisbee]]: "dog" or "dogs", and "frisbee" -- or a list of N such lists; at most 3 sets of at most 4 alternative
    token ids in [1, V), disjoint within an image and not banned.  An image owns 2^sets * beam_width rows of the decode.  Returns what
    beam_nbest_batch returns; an image whose sets could not be met within nword words has fewer than beam_width entries, possibly none.
    With no sets it is beam_constrained_batch, bit for bit."""
    N, K, L = feats.shape[0], beam_width, nword + 2
    out = (C.c_int32 * (N * K * L))()
    n = (C.c_int * (N * K))()
    lp = (C.c_float * (N * K))()
    sc = (C.c_float * (N * K))()
    cons, keep = _constraints(banned, min_len, no_repeat_ngram)
    fw, keep_words, _ = _forced(forced, N)
    ctx._call("lrcn_beam_forced_batch", _p9(param), _ptr(feats), N, K, nword, float(alpha), C.byref(cons), C.byref(fw) if fw is not None else None,
              out, n, lp, sc)
    del keep, keep_words
    toks = np.ctypeslib.as_array(out).reshape(N * K, L).tolist()
    n, lp, sc = list(n), list(lp), list(sc)
    return [[(toks[r][:n[r]], lp[r], sc[r]) for r in range(i * K, (i + 1) * K) if n[r] > 0] for i in range(N)]


def forced_captions(ctx, param, feats, index_to_word, beam_width, nword, alpha=0.0, forced=(), banned=(), min_len=0, no_repeat_ngram=0,
                    normalize=False):
    """beam_forced_batch as caption text: as nbest_captions."""
    if normalize:
        f = from_jl(feats)
        feats = to_jl(f / f.sum(axis=1, keepdims=True))  # input/sum(input) per image (lrcn.jl:597)
    res = beam_forced_batch(ctx, param, feats, beam_width, nword, alpha, forced, banned, min_len, no_repeat_ngram)
    return [[(_caption(toks, index_to_word), lp, sc) for toks, lp, sc in entries] for entries in res]


def forced_topk_logits(ctx, logits, K, hist, current, words, banned=(), min_len=0, no_repeat_ngram=0):
    """One step of the forced-word top-K on the caller's own logits (lrcn_forced_topk_logits, include/lrcn_forced.h): logits and hist as
    constrained_topk_logits; words int [R][C][A] (one row per "image", -1: no word; C may be 0) -> numpy (stay columns [R][K] int32, their
    logp [R][K] f32, move logp [R][C*A] f32, states [R] int32).  Independent of the context's model sizes."""
    dev = "cuda:%d" % ctx.device
    if isinstance(logits, torch.Tensor):
        z = logits
    else:
        a = np.ascontiguousarray(logits, dtype=np.float32)
        ld = (a.shape[1] + 3) // 4 * 4   # rows 16 bytes apart
        z = torch.zeros((a.shape[0], ld), dtype=torch.float32, device=dev)[:, :a.shape[1]]
        z.copy_(torch.from_numpy(a))
    R, V = z.shape
    w = np.ascontiguousarray(words, dtype=np.int32)
    if w.ndim != 3 or w.shape[0] != R:
        raise LrcnError("forced words: an int array [R][C][A]")
    Cn, An = w.shape[1], w.shape[2]
    h = torch.from_numpy(np.ascontiguousarray(hist, dtype=np.int32)).to(dev)
    idx = torch.empty((R, K), dtype=torch.int32, device=z.device)
    lp = torch.empty((R, K), dtype=torch.float32, device=z.device)
    mv = torch.empty((R, max(Cn * An, 1)), dtype=torch.float32, device=z.device)
    st = torch.empty(R, dtype=torch.int32, device=z.device)
    cons, keep = _constraints(banned, min_len, no_repeat_ngram)
    torch.cuda.synchronize(z.device)   # the uploads have landed whichever stream the context runs on
    ctx._call("lrcn_forced_topk_logits", C.c_void_p(z.data_ptr()), z.stride(0), R, V, int(K), C.byref(cons),
              w.ctypes.data_as(C.POINTER(C.c_int32)), Cn, An, C.c_void_p(h.data_ptr()), h.shape[1], int(current), C.c_void_p(idx.data_ptr()),
              C.c_void_p(lp.data_ptr()), C.c_void_p(mv.data_ptr()), C.c_void_p(st.data_ptr()))
    del keep
    ctx.sync()
    return idx.cpu().numpy(), lp.cpu().numpy(), mv.cpu().numpy()[:, :Cn * An], st.cpu().numpy()


_ENSEMBLE_MODES = {"prob": 0, "logprob": 1}   # LRCN_ENSEMBLE_PROB / LRCN_ENSEMBLE_LOGPROB


def _ensemble_args(M, weights, mode):
    """-> (float array of M weights or None for uniform, the mode's number); the library checks the values"""
    if mode not in _ENSEMBLE_MODES:
        raise LrcnError("ensemble mode %r: 'prob' or 'logprob'" % (mode,))
    if weights is None:
        return None, _ENSEMBLE_MODES[mode]
    w = [float(x) for x in weights]
    if len(w) != M:
        raise LrcnError("%d ensemble weights for %d members" % (len(w), M))
    return (C.c_float * M)(*w), _ENSEMBLE_MODES[mode]


def ensemble_mix_logits(ctx, logits_list, weights=None, mode="prob", out=None):
    """The mixture rows of M members' logits (lrcn_ensemble_mix_logits, include/lrcn_ensemble.h): each member numpy [R][V] f32 or a torch
    device tensor [R][V] f32 with any row stride >= V and unit column stride -> numpy [R][V] f32.  mode 'prob': the log of the weighted
    mean of the members' softmax rows; 'logprob': the weighted sum of their log-softmax rows.  Independent of the context's model sizes.
    out: a device tensor [R][V] f32 of the same kind to write into (default: rows 16 bytes apart)."""
    dev = "cuda:%d" % ctx.device
    zs = []
    for z in logits_list:
        if not isinstance(z, torch.Tensor):
            z = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).to(dev)
        if z.dtype != torch.float32 or z.dim() != 2 or z.stride(1) != 1:
            raise LrcnError("ensemble logits: [R][V] float32 with unit column stride")
        zs.append(z)
    M = len(zs)
    if M < 1 or any(z.shape != zs[0].shape for z in zs):
        raise LrcnError("ensemble logits: at least one member, all of one shape")
    R, V = zs[0].shape
    w, md = _ensemble_args(M, weights, mode)
    if out is None:
        out = torch.empty((R, (V + 3) // 4 * 4), dtype=torch.float32, device=zs[0].device)[:, :V]   # rows 16 bytes apart
    elif out.dtype != torch.float32 or tuple(out.shape) != (R, V) or out.stride(1) != 1 or not out.is_cuda:
        raise LrcnError("ensemble out: a device tensor [R][V] float32 with unit column stride")
    ptrs = (C.c_void_p * M)(*[z.data_ptr() for z in zs])
    lds = (C.c_int64 * M)(*[z.stride(0) for z in zs])
    torch.cuda.synchronize(zs[0].device)   # the uploads have landed whichever stream the context runs on
    ctx._call("lrcn_ensemble_mix_logits", ptrs, lds, M, w, md, R, V, C.c_void_p(out.data_ptr()), out.stride(0))
    ctx.sync()
    return out.cpu().numpy()


def beam_ensemble_batch(ctxs, params, feats, beam_width, nword, alpha=0.0, weights=None, mode="prob", banned=(), min_len=0, no_repeat_ngram=0,
                        groups=0, strength=0.0):
    """Ensemble beam search (lrcn_beam_ensemble_batch, include/lrcn_ensemble.h): member m is the context ctxs[m] with the model params[m];
    every step the members' next-word distributions are mixed (mode 'prob': weighted arithmetic mean, 'logprob': weighted geometric mean;
    weights None: uniform) and beam_constrained_batch's search runs on the mixture.  The members share the vocabulary, the device and the
    stream and may differ in everything else.  Returns what beam_constrained_batch returns; logp is the mixture's log-likelihood."""
    M = len(ctxs)
    if M < 1 or len(params) != M:
        raise LrcnError("ensemble: %d contexts, %d models" % (M, len(params)))
    N, K, G, L = feats.shape[0], beam_width, int(groups), nword + 2
    out = (C.c_int32 * (N * K * L))()
    n = (C.c_int * (N * K))()
    lp = (C.c_float * (N * K))()
    sc = (C.c_float * (N * K))()
    cons, keep = _constraints(banned, min_len, no_repeat_ngram)
    w, md = _ensemble_args(M, weights, mode)
    p9s = [_p9(p) for p in params]
    hs = (C.c_void_p * M)(*[c._h.value for c in ctxs])
    ps = (C.c_void_p * M)(*[C.addressof(p) for p in p9s])
    rc = _lib.lib().lrcn_beam_ensemble_batch(hs, ps, M, w, md, _ptr(feats), N, K, G, float(strength), nword, float(alpha), C.byref(cons), out, n,
                                             lp, sc)
    _lib.check(ctxs[0]._h, rc)
    del keep, p9s
    toks = np.ctypeslib.as_array(out).reshape(N * K, L).tolist()
    n, lp, sc = list(n), list(lp), list(sc)
    if G == 0:
        return [[(toks[r][:n[r]], lp[r], sc[r]) for r in range(i * K, (i + 1) * K) if n[r] > 0] for i in range(N)]
    Kp = K // G
    return [[[(toks[r][:n[r]], lp[r], sc[r]) for r in range(i * K + g * Kp, i * K + (g + 1) * Kp) if n[r] > 0] for g in range(G)] for i in range(N)]


def ensemble_captions(ctxs, params, feats, index_to_word, beam_width, nword, alpha=0.0, weights=None, mode="prob", banned=(), min_len=0,
                      no_repeat_ngram=0, groups=0, strength=0.0, normalize=False):
    """beam_ensemble_batch as caption text: as constrained_captions."""
    if normalize:
        f = from_jl(feats)
        feats = to_jl(f / f.sum(axis=1, keepdims=True))  # input/sum(input) per image (lrcn.jl:597)
    res = beam_ensemble_batch(ctxs, params, feats, beam_width, nword, alpha, weights, mode, banned, min_len, no_repeat_ngram, groups, strength)
    if groups == 0:
        return [[(_caption(toks, index_to_word), lp, sc) for toks, lp, sc in entries] for entries in res]
    return [[[(_caption(toks, index_to_word), lp, sc) for toks, lp, sc in grp] for grp in img] for img in res]


def _caption(seq, index_to_word):
    words = []
    for t in seq[1:]:
        if t == EOS:
            break
        words.append(index_to_word[t])
    return " ".join(words + ["."])


def sample_captions(ctx, param, feats, index_to_word, nsamples, nword, temperature=1.0, top_k=0, seed=0, normalize=False, top_p=1.0):
    """sample_batch as caption text (as generate): per image the nsamples captions, highest log-likelihood first (ties: sample order)."""
    if normalize:
        f = from_jl(feats)
        feats = to_jl(f / f.sum(axis=1, keepdims=True))  # input/sum(input) per image (lrcn.jl:597)
    res = []
    for samples in sample_batch(ctx, param, feats, nsamples, nword, temperature, top_k, seed, top_p=top_p):
        order = sorted(range(len(samples)), key=lambda s: -samples[s][1])
        res.append([_caption(samples[s][0], index_to_word) for s in order])
    return res


def _score_args(feats, captions, normalize):
    """captions (lists of 0-based ids, no bos / eos) -> host tokens [Tmax][M], lens [M]; feats normalised per image if asked (lrcn.jl:597)."""
    if normalize:
        f = from_jl(feats)
        feats = to_jl(f / f.sum(axis=1, keepdims=True))
    M = len(captions)
    lens = np.array([len(c) for c in captions], np.int32)
    Tmax = max(1, int(lens.max())) if M else 1
    tok = np.zeros((Tmax, max(M, 1)), np.int32)
    for m, cap in enumerate(captions):
        tok[:len(cap), m] = cap
    return feats, np.ascontiguousarray(tok), lens, Tmax


def score_matrix(ctx, param, feats, captions, normalize=False):
    """s(n, m) = log p(caption m | image n) summed over its words and eos (lrcn_score_matrix, include/lrcn_score.h; paper section 5.1):
    feats N x 4096, captions M lists of 0-based token ids without bos / eos -> numpy float32 N x M."""
    feats, tok, lens, Tmax = _score_args(feats, captions, normalize)
    N, M = feats.shape[0], len(captions)
    out = torch.empty(N * max(M, 1), dtype=torch.float32, device=feats.device)
    ctx._call("lrcn_score_matrix", _p9(param), _ptr(feats), N, tok.ctypes.data_as(C.POINTER(C.c_int32)),
              lens.ctypes.data_as(C.POINTER(C.c_int)), M, Tmax, C.c_void_p(out.data_ptr()))
    ctx.sync()
    return out.cpu().numpy().reshape(M, N).T.copy()


def score_pairs(ctx, param, feats, captions, pair_img, pair_cap, normalize=False):
    """score_matrix at the P given (image, caption) pairs only (lrcn_score_pairs) -> numpy float32 [P]."""
    feats, tok, lens, Tmax = _score_args(feats, captions, normalize)
    pi = np.ascontiguousarray(pair_img, dtype=np.int32)
    pc = np.ascontiguousarray(pair_cap, dtype=np.int32)
    if pi.shape != pc.shape or pi.ndim != 1:
        raise LrcnError("pair_img and pair_cap must be 1-D and of one length")
    out = torch.empty(max(len(pi), 1), dtype=torch.float32, device=feats.device)
    ctx._call("lrcn_score_pairs", _p9(param), _ptr(feats), feats.shape[0], tok.ctypes.data_as(C.POINTER(C.c_int32)),
              lens.ctypes.data_as(C.POINTER(C.c_int)), len(captions), Tmax, pi.ctypes.data_as(C.POINTER(C.c_int32)),
              pc.ctypes.data_as(C.POINTER(C.c_int32)), len(pi), C.c_void_p(out.data_ptr()))
    ctx.sync()
    return out.cpu().numpy()[:len(pi)].copy()


def generate(ctx, param, feat, index_to_word, nword, beam_width, normalize=False):
    """generate (lrcn.jl:585-642): caption text "w1 w2 ... ." -- words after bos up to the first eos (:634-640)."""
    if normalize:
        feat = to_jl(from_jl(feat) / from_jl(feat).sum())  # input/sum(input) (lrcn.jl:597)
    seq, _ = beam_search(ctx, param, feat, beam_width, nword)
    return _caption(seq, index_to_word)


# ------------------------------------------------------------------------------------------------ VGG
def vgg_load(ctx, conv_w, conv_b, fc6, fc7):
    """get_params_cnn's output (lrcn.jl:697-721) -> the context. conv_w[l]: (3,3,Cin,Cout) column-major tensors."""
    cw = _lib.P13(*[_ptr(t).value for t in conv_w])
    cb = _lib.P13(*[_ptr(t).value for t in conv_b])
    ctx._call("lrcn_vgg_load", cw, cb, _ptr(fc6[0]), _ptr(fc6[1]), _ptr(fc7[0]), _ptr(fc7[1]))


def convnet(ctx, x):
    """convnet(xs) (lrcn.jl:734-747): x (224,224,3,N) column-major -> feats N x 4096."""
    N = x.shape[3]
    feats = jl_empty(N, CNNOUT)
    ctx._call("lrcn_vgg_forward", _ptr(x), N, _ptr(feats))
    return feats


def convnet_u8(ctx, img_u8, mean=VGG_MEAN, feats=None, normalize=False):
    """Fused read_image_data arithmetic (lrcn.jl:766-772) + convnet on uint8 crops img[n][row][col][c].  mean=None: the
    averageImage registered with set_average_image.  normalize: divide each feature row by its sum (lrcn.jl:595-597)."""
    if torch.is_tensor(img_u8) and not img_u8.is_cuda:  # host crops: through the staging buffers (asynchronous when pinned)
        img_u8 = upload_crops(ctx, img_u8)
    N = img_u8.shape[0]
    if feats is None:
        feats = jl_empty(N, CNNOUT)
    m = (C.c_float * 3)(*mean) if mean is not None else None
    ctx._call("lrcn_vgg_forward_u8", C.c_void_p(img_u8.data_ptr()), N, m, _ptr(feats))
    if normalize:
        normalize_features(ctx, feats)
    return feats


def convnet_u8_blocks(ctx, img_u8, block_rows, mean=VGG_MEAN, feats=None, normalize=False):
    """The VGG forward for the crops of m = N / block_rows training batches at once (lrcn_vgg_forward_u8_blocks) -> list of m feature
    tensors block_rows x 4096 (column-major views into one buffer `feats` of m * block_rows * 4096 floats)."""
    if torch.is_tensor(img_u8) and not img_u8.is_cuda:
        img_u8 = upload_crops(ctx, img_u8)
    N = img_u8.shape[0]
    m = N // block_rows
    if feats is None:
        feats = torch.empty(m * block_rows * CNNOUT, device="cuda", dtype=torch.float32)
    mm = (C.c_float * 3)(*mean) if mean is not None else None
    ctx._call("lrcn_vgg_forward_u8_blocks", C.c_void_p(img_u8.data_ptr()), N, mm, int(block_rows), int(bool(normalize)), C.c_void_p(feats.data_ptr()))
    n = block_rows * CNNOUT
    return [feats[b * n:(b + 1) * n].view(CNNOUT, block_rows).permute(1, 0) for b in range(m)]


class StagedCrops:
    """uint8 crops [N][224][224][3] in one of the context's two device staging buffers (lrcn_upload_crops): stands wherever a device crop
    tensor does (convnet_u8, train_step_dp).  `host` keeps the source buffer alive until the asynchronous copy has certainly been issued
    AND consumed (the trainer drops it after the forward that reads the staging buffer has been queued)."""

    def __init__(self, ptr, N, host):
        self.ptr, self.shape, self.host = int(ptr), (int(N), 224, 224, 3), host
        self.is_cuda = True

    def data_ptr(self):
        return self.ptr


def upload_crops(ctx, host_u8):
    """The per-batch host -> device copy of the training loop (lrcn.jl:369-376) off the critical path: `host_u8` (CPU uint8 tensor
    [N][224][224][3]; pinned = a true asynchronous DMA) is copied on the context's copy stream into a device staging buffer.  Returns at
    once; the forward that is handed the result waits on the device (include/lrcn.h "input feed")."""
    if host_u8.is_cuda or host_u8.dtype != torch.uint8 or not host_u8.is_contiguous() or tuple(host_u8.shape[1:]) != (224, 224, 3):
        raise LrcnError("upload_crops takes a contiguous CPU uint8 tensor [N][224][224][3]")
    out = C.c_void_p()
    ctx._call("lrcn_upload_crops", C.c_void_p(host_u8.data_ptr()), int(host_u8.shape[0]), C.byref(out))
    return StagedCrops(out.value, host_u8.shape[0], host_u8)


def upload_wait(ctx):
    """Block until every upload issued so far has run (a loader calls it before refilling a pinned buffer)."""
    ctx._call("lrcn_upload_wait")


def read_image_data_u8(ctx, img_u8, mean=VGG_MEAN):
    """read_image_data's arithmetic tail (lrcn.jl:766-772) -> (224,224,3,N) column-major float tensor."""
    N = img_u8.shape[0]
    out = jl_empty(224, 224, 3, N)
    m = (C.c_float * 3)(*mean) if mean is not None else None
    ctx._call("lrcn_preprocess_u8", C.c_void_p(img_u8.data_ptr()), N, m, _ptr(out))
    return out


def set_average_image(ctx, average_image):
    """Register the VGG averageImage (lrcn.jl:113), a (224,224,3) array, or None to go back to per-channel means."""
    if average_image is None:
        ctx._call("lrcn_set_average_image", None)
        return
    a = to_jl(np.asarray(average_image, np.float32).reshape(224, 224, 3))
    ctx._call("lrcn_set_average_image", _ptr(a))
    ctx.sync()  # `a` may be freed on return


def resize_crop_u8(ctx, images):
    """read_image_data's geometry (lrcn.jl:755-765) on the GPU for a list of decoded images (uint8 arrays [h][w], [h][w][1],
    [h][w][3] or [h][w][4]) of any sizes -> uint8 crops tensor [N][224][224][3] on the device (lrcn_resize_crop_u8)."""
    arrs = [np.ascontiguousarray(np.asarray(im, dtype=np.uint8)) for im in images]
    arrs = [a[:, :, None] if a.ndim == 2 else a for a in arrs]
    N = len(arrs)
    offs = np.zeros(N, np.int64)
    pos = 0
    for i, a in enumerate(arrs):
        offs[i] = pos
        pos += a.size
    flat = torch.as_tensor(np.concatenate([a.reshape(-1) for a in arrs])).cuda()
    hs = (C.c_int * N)(*[a.shape[0] for a in arrs])
    ws = (C.c_int * N)(*[a.shape[1] for a in arrs])
    cs = (C.c_int * N)(*[a.shape[2] for a in arrs])
    out = torch.empty((N, 224, 224, 3), dtype=torch.uint8, device=flat.device)
    ctx._call("lrcn_resize_crop_u8", C.c_void_p(flat.data_ptr()), offs.ctypes.data_as(C.POINTER(C.c_int64)), hs, ws, cs, N,
              C.c_void_p(out.data_ptr()))
    ctx.sync()  # `flat` may be freed on return
    return out


def normalize_features(ctx, feats):
    """feats (N x 4096, column-major) <- rows divided by their sums, in place: generate's input/sum(input) (lrcn.jl:595-597)."""
    ctx._call("lrcn_normalize_features", _ptr(feats), feats.shape[0])
    return feats


def conv3x3(ctx, x, w, b, relu=True, pool=False):
    """convx/relux/poolx probe (lrcn.jl:724-726) in reference layouts."""
    W, H, Cin, N = x.shape
    Cout = w.shape[3]
    y = jl_empty(W // 2 if pool else W, H // 2 if pool else H, Cout, N)
    ctx._call("lrcn_conv3x3", _ptr(x), W, H, Cin, N, _ptr(w), _ptr(b), Cout, int(relu), int(pool), _ptr(y))
    return y


def conv1_fused(ctx, img_u8, mean, w11, b11, w12, b12):
    """The bf16 stack's first launch as a probe (conv64f.hip): crops [N][S][S][3] uint8 (device) -> pool1 (S/2, S/2, 64, N); w11 (3,3,3,64),
    w12 (3,3,64,64) in the reference layouts (lrcn.jl:770 + 724-726 twice)."""
    N, S = img_u8.shape[0], img_u8.shape[1]
    y = jl_empty(S // 2, S // 2, 64, N)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    ctx._call("lrcn_conv1_fused", C.c_void_p(img_u8.data_ptr()), N, S, m, _ptr(w11), _ptr(b11), _ptr(w12), _ptr(b12), _ptr(y))
    return y


def debug_conv11(ctx, src, w11, b11, mean=VGG_MEAN):
    """conv1_1 of the bf16 stack by itself (lrcn_debug_conv11, include/lrcn_conv_debug.h; conv11.hip).  src: uint8 crops [N][S][S][3] (device;
    `mean` is subtracted per channel) or the preprocessed float tensor (S,S,3,N) column-major (`mean` is not used) -> (S,S,64,N)."""
    if src.dtype == torch.uint8:
        N, S, u8 = src.shape[0], src.shape[1], 1
        m = (C.c_float * 3)(*[float(v) for v in mean])
    else:
        S, N, u8, m = src.shape[0], src.shape[3], 0, None
    y = jl_empty(S, S, 64, N)
    ctx._call("lrcn_debug_conv11", C.c_void_p(src.data_ptr()) if u8 else _ptr(src), u8, N, S, m, _ptr(w11), _ptr(b11), _ptr(y))
    return y


def debug_fp8_cast(ctx, src, factor, to_fp8):
    """One of fp8.hip's two casts (lrcn_debug_fp8_cast, include/lrcn_conv_debug.h) on a flat device tensor: to_fp8 -- bfloat16 [n] -> e4m3
    bytes (uint8 [n]) = e4m3(clamp(src * factor)); otherwise e4m3 bytes (uint8 [n]) -> bfloat16 [n] = bf16(src * factor)."""
    if src.dtype != (torch.bfloat16 if to_fp8 else torch.uint8) or src.dim() != 1 or not src.is_cuda or not src.is_contiguous():
        raise LrcnError("debug_fp8_cast takes a flat device tensor, bfloat16 towards e4m3 and uint8 from it")
    dst = torch.empty(src.numel(), dtype=torch.uint8 if to_fp8 else torch.bfloat16, device=src.device)
    ctx._call("lrcn_debug_fp8_cast", 0 if to_fp8 else 1, C.c_void_p(src.data_ptr()), src.numel(), float(factor), C.c_void_p(dst.data_ptr()))
    return dst


def debug_amax(ctx, x_bf16, out=None):
    """max |x| of a flat bfloat16 device tensor through the calibration pass's kernel (lrcn_debug_amax) -> one-element float32 device
    tensor (`out`, if given, is overwritten: the entry zeroes it first)."""
    if x_bf16.dtype != torch.bfloat16 or not x_bf16.is_cuda or not x_bf16.is_contiguous():
        raise LrcnError("debug_amax takes a contiguous bfloat16 device tensor")
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=x_bf16.device)
    ctx._call("lrcn_debug_amax", C.c_void_p(x_bf16.data_ptr()), x_bf16.numel(), C.c_void_p(out.data_ptr()))
    return out


def debug_conv64_f8(ctx, x, w, b, f8_inv_scale):
    """conv2_1's e4m3 epilogue by itself (lrcn_debug_conv64_f8; conv64.hip with f8_inv_scale > 0): x (W,H,64,N), w (3,3,64,Cout), b [Cout]
    -> (W,H,Cout,N) holding the e4m3 values e4m3(min(relu(conv + b) * f8_inv_scale, 448)), undequantised."""
    W, H, Cin, N = x.shape
    if Cin != 64:
        raise LrcnError("debug_conv64_f8: Cin must be 64")
    Cout = w.shape[3]
    y = jl_empty(W, H, Cout, N)
    ctx._call("lrcn_debug_conv64_f8", _ptr(x), W, H, N, _ptr(w), _ptr(b), Cout, float(f8_inv_scale), _ptr(y))
    return y


def debug_fp8_scales(ctx):
    """The 13 per-layer activation scales of the last lrcn_vgg_calibrate (lrcn_debug_fp8_scales) as a float32 array; 0 below conv2_1."""
    out = (C.c_float * 13)()
    ctx._call("lrcn_debug_fp8_scales", out)
    return np.array(out[:], dtype=np.float32)


def vgg_set_wg_cap(ctx, cap):
    """Cap the VGG convolution grids at `cap` workgroups (0 = off): include/lrcn.h lrcn_vgg_set_wg_cap."""
    ctx._call("lrcn_vgg_set_wg_cap", int(cap))


def vgg_calibrate(ctx, img_u8, mean=VGG_MEAN, margin=1.25):
    """vgg_dtype = LRCN_FP8 only: one bf16 pass over `img_u8` (uint8 crops [n][row][col][c]) that fixes the per-layer
    activation scales of the e4m3 layers (include/lrcn.h lrcn_vgg_calibrate).  No counterpart in the reference."""
    m = (C.c_float * 3)(*mean) if mean is not None else None
    ctx._call("lrcn_vgg_calibrate", C.c_void_p(img_u8.data_ptr()), img_u8.shape[0], m, float(margin))


def conv3x3_fp8(ctx, x, w, b, sa_in, sa_out, relu=True, pool=False):
    """e4m3 probe of one layer (include/lrcn.h lrcn_conv3x3_fp8) -> (y dequantised, per-channel weight scales)."""
    W, H, Cin, N = x.shape
    Cout = w.shape[3]
    y = jl_empty(W // 2 if pool else W, H // 2 if pool else H, Cout, N)
    sw = torch.empty(Cout, dtype=torch.float32, device=x.device)
    ctx._call("lrcn_conv3x3_fp8", _ptr(x), W, H, Cin, N, _ptr(w), _ptr(b), Cout, int(relu), int(pool), float(sa_in), float(sa_out),
              _ptr(y), C.c_void_p(sw.data_ptr()))
    return y, sw


def debug_route(ctx, which=0):
    """Kernel family of the last contraction (which=0) / per layer of the last VGG forward (which=1): lrcn_debug_route."""
    r = _lib.lib().lrcn_debug_route(ctx._h, int(which))
    return r.decode() if r else ""


def debug_gemm(ctx, dtype, A, B, Cmat, M, N, K, lda, ldb, ldc, bias=None, c_f32=False, beta=False, relu=False, c_is_zero=False,
               deterministic=False, free_cus=0, bg_cus=0, wg_cap=0):
    """C[M][N] (+)= A[M][K] B[N][K]^T (+ bias) (ReLU) through the GEMM router on the caller's device operands (lrcn_debug_gemm,
    include/lrcn_gemm_debug.h): A, B, Cmat, bias are device tensors already in their element type (sub-views welcome: data_ptr() is what
    goes down) or raw addresses (int / None); leading dimensions in elements.  Returns the route that ran (debug_route(ctx, 0))."""
    def addr(t):
        if t is None:
            return None
        if torch.is_tensor(t):
            if not t.is_cuda:
                raise LrcnError("expected a CUDA (HIP) tensor")
            return C.c_void_p(t.data_ptr())
        return C.c_void_p(int(t))
    g = _lib.GemmDebug(int(dtype), addr(A), addr(B), addr(Cmat), addr(bias), int(lda), int(ldb), int(ldc), int(M), int(N), int(K),
                       int(bool(c_f32)), int(bool(beta)), int(bool(relu)), int(bool(c_is_zero)), int(bool(deterministic)),
                       int(free_cus), int(bg_cus), int(wg_cap))
    ctx._call("lrcn_debug_gemm", C.byref(g))
    return debug_route(ctx, 0)


def debug_conv_gemm(ctx, dtype, x, w, y, N, H, W, Cin, Cout, ldc, bias=None, relu=False, pool=False, wg_cap=0):
    """One 3x3 convolution (+ bias) (ReLU) (2x2 maximum) through the GEMM router's CONV3 mode on the caller's device operands
    (lrcn_debug_conv_gemm, include/lrcn_gemm_debug.h): x NHWC [N][H][W][Cin], w [Cout][9][Cin], y [N][H][W] (pooled: [N][H/2][W/2]) rows
    of ldc elements, all in the element type `dtype` names; bias f32.  Device tensors (sub-views welcome: data_ptr() is what goes down) or
    raw addresses (int / None).  Returns the route that ran (debug_route(ctx, 0))."""
    def addr(t):
        if t is None:
            return None
        if torch.is_tensor(t):
            if not t.is_cuda:
                raise LrcnError("expected a CUDA (HIP) tensor")
            return C.c_void_p(t.data_ptr())
        return C.c_void_p(int(t))
    g = _lib.ConvGemmDebug(int(dtype), addr(x), addr(w), addr(bias), addr(y), int(ldc), int(N), int(H), int(W), int(Cin), int(Cout),
                           int(bool(relu)), int(bool(pool)), int(wg_cap))
    ctx._call("lrcn_debug_conv_gemm", C.byref(g))
    return debug_route(ctx, 0)


def debug_conv64(ctx, x, w, y, N, H, W, Cout, bias=None, relu=False, pool=False, wg_cap=0):
    """One 3x3 convolution of 64 input channels (+ bias) (ReLU) (2x2 maximum) on conv64.hip's halo-patch kernel, on the caller's device
    operands (lrcn_debug_conv64, include/lrcn_conv_debug.h): x bfloat16 NHWC [N][H][W][64], w bfloat16 [Cout][9][64], y bfloat16
    [N][H][W][Cout] (pooled: [N][H/2][W/2][Cout]), bias float32 or None; wg_cap as lrcn_vgg_set_wg_cap's.  Device tensors (sub-views welcome:
    data_ptr() is what goes down) or raw addresses (int / None).  Returns the route that ran (debug_route(ctx, 0))."""
    def addr(t):
        if t is None:
            return None
        if torch.is_tensor(t):
            if not t.is_cuda:
                raise LrcnError("expected a CUDA (HIP) tensor")
            return C.c_void_p(t.data_ptr())
        return C.c_void_p(int(t))
    d = _lib.Conv64Debug(addr(x), addr(w), addr(bias), addr(y), int(N), int(H), int(W), int(Cout), int(bool(relu)), int(bool(pool)), int(wg_cap))
    ctx._call("lrcn_debug_conv64", C.byref(d))
    return debug_route(ctx, 0)


def debug_decode_steps(ctx, param, feats, per_image, tokens, parents, out=None):
    """The batched decode step on caller-given tokens and parents (lrcn_debug_decode_steps, include/lrcn_decode_debug.h): feats N x 4096 on
    the device, tokens / parents [steps][N * per_image] host ints (row r of step s feeds tokens[s][r] and continues the states row
    parents[s][r] had after step s-1; parents[0] is not read).  Returns a dict of NumPy arrays -- "h1", "c1", "h2", "c2" [steps][R][H] (h2,
    c2 None on LRCN-1f), "logits" [steps][R][V], float32, a bfloat16 h widened on the host -- and "route": 0 plain, 1 cell epilogue, 2 tables.
    out: the device tensors the call writes ("h1", "h2" in the LSTM element type, "c1", "c2", "logits" float32) instead of fresh ones."""
    tok = np.ascontiguousarray(np.asarray(tokens, dtype=np.int32))
    par = np.ascontiguousarray(np.asarray(parents, dtype=np.int32))
    N = feats.shape[0]
    R = N * int(per_image)
    if tok.ndim != 2 or tok.shape != par.shape or tok.shape[1] != R:
        raise LrcnError("tokens and parents must both be [steps][N * per_image]")
    S, two = tok.shape[0], ctx.n_layers != 1
    ht = torch.bfloat16 if ctx.lstm_dtype == LRCN_BF16 else torch.float32
    dev = feats.device
    if out is None:
        out = {"h1": torch.empty((S, R, ctx.H1), dtype=ht, device=dev), "c1": torch.empty((S, R, ctx.H1), dtype=torch.float32, device=dev),
               "h2": torch.empty((S, R, ctx.H2), dtype=ht, device=dev) if two else None,
               "c2": torch.empty((S, R, ctx.H2), dtype=torch.float32, device=dev) if two else None,
               "logits": torch.empty((S, R, ctx.V), dtype=torch.float32, device=dev)}
    addr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    p9 = _p9(param)
    d = _lib.DecodeDebug(C.cast(p9, C.POINTER(C.c_void_p)), _ptr(feats), N, int(per_image), S, tok.ctypes.data_as(C.POINTER(C.c_int32)),
                         par.ctypes.data_as(C.POINTER(C.c_int32)), addr(out["h1"]), addr(out.get("h2")), addr(out["c1"]), addr(out.get("c2")),
                         addr(out["logits"]), -1)
    ctx._call("lrcn_debug_decode_steps", C.byref(d))
    def host(t):   # copied as stored; bfloat16 bits widened to float32 here, on the host
        if t is None:
            return None
        if t.dtype == torch.bfloat16:
            bits = t.view(torch.int16).cpu().numpy().view(np.uint16).astype(np.uint32) << 16
            return bits.view(np.float32)
        return t.cpu().numpy()
    res = {k: host(out.get(k)) for k in ("h1", "c1", "h2", "c2", "logits")}
    res["route"] = d.route
    return res


def synthetic_vgg_weights(seed=1, device="cuda", bias_std=0.0):
    """He-normal(fan_in) VGG-16 weights (no pretrained file offline); biases zero, or N(0, bias_std)
    so that every bias path of the kernels sees non-zero values (parity tests)."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    conv_w, conv_b = [], []
    cin = 3
    for cout in VGG_COUT:
        w = jl_empty(3, 3, cin, cout, device=device)
        w.copy_(torch.randn((3, 3, cin, cout), generator=g, device=device) * float(np.sqrt(2.0 / (9 * cin))))
        conv_w.append(w)
        conv_b.append(torch.randn(cout, generator=g, device=device) * bias_std if bias_std else torch.zeros(cout, device=device))
        cin = cout
    fc6 = jl_empty(4096, 25088, device=device)
    fc6.copy_(torch.randn((4096, 25088), generator=g, device=device) * float(np.sqrt(2.0 / 25088)))
    fc7 = jl_empty(4096, 4096, device=device)
    fc7.copy_(torch.randn((4096, 4096), generator=g, device=device) * float(np.sqrt(2.0 / 4096)))
    b6 = torch.randn(4096, generator=g, device=device) * bias_std if bias_std else torch.zeros(4096, device=device)
    b7 = torch.randn(4096, generator=g, device=device) * bias_std if bias_std else torch.zeros(4096, device=device)
    return conv_w, conv_b, (fc6, b6), (fc7, b7)
