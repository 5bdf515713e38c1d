"""Activity recognition (paper section 4) over the C ABI of include/lrcn_activity.h: one LSTM layer over per-frame features, a softmax
over the action classes at every step, a clip's prediction the mean of its per-step distributions and a video's the mean over its clips.

Arrays are torch CUDA tensors in the reference's column-major memory (lrcn.jl_empty / to_jl): the model is four tensors
W (F+H) x 4H, b 1 x 4H, Wout H x C, bout 1 x C; a batch of B clips of T frames is a (B*T) x F feature matrix, row b*T + t.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import LRCN_BF16, LRCN_F32, LrcnError  # noqa: F401
from .lrcn import _ptr, from_jl, jl_empty, jl_zeros, to_jl

PARAM_NAMES = ("W", "b", "Wout", "bout")


def param_shapes(F, H, C_):
    return [(F + H, 4 * H), (1, 4 * H), (H, C_), (1, C_)]


def clips(n_frames, T=16, stride=8):
    """The clips of a video of n_frames frames: (start, length) pairs, windows of T frames every `stride` frames (the paper's 16 / 8).
    A video shorter than T is one clip of all its frames; a tail the windows miss gets one more window that ends at the last frame."""
    n_frames, T, stride = int(n_frames), int(T), int(stride)
    if n_frames < 1 or T < 1 or stride < 1:
        raise LrcnError("clips: n_frames, T and stride must be >= 1")
    if n_frames <= T:
        return [(0, n_frames)]
    out = [(s, T) for s in range(0, n_frames - T + 1, stride)]
    if out[-1][0] + T < n_frames:
        out.append((n_frames - T, T))
    return out


def gather_clips(video_feats, specs, T):
    """Host batch of clips: video_feats[i] is an [n_frames_i x F] array; specs a list of (video index, start, length).
    -> (feats [B*T x F] float32, row b*T + t; zeros past each clip's length), lens int32 [B])."""
    F = video_feats[specs[0][0]].shape[1]
    out = np.zeros((len(specs) * T, F), np.float32)
    lens = np.zeros(len(specs), np.int32)
    for b, (v, s, n) in enumerate(specs):
        out[b * T:b * T + n] = video_feats[v][s:s + n]
        lens[b] = n
    return out, lens


class ActivityModel:
    """One lrcn_act handle with its model, gradients and Adam state (all device tensors owned here)."""

    def __init__(self, F, H, C_, max_B, max_T=16, dtype=LRCN_F32, deterministic=False, device=None, seed=1):
        if not torch.cuda.is_available():
            raise LrcnError("no MI355X visible: liblrcn_hip has no CPU path")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.F, self.H, self.C, self.max_B, self.max_T = int(F), int(H), int(C_), int(max_B), int(max_T)
        self.dtype, self.deterministic = int(dtype), bool(deterministic)
        cfg = _lib.ActConfig(self.device, self.F, self.H, self.C, self.max_B, self.max_T, self.dtype, int(self.deterministic))
        h = C.c_void_p()
        rc = _lib.lib().lrcn_act_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            msg = _lib.lib().lrcn_act_last_error(None)
            raise LrcnError("lrcn_act_create error %d: %s" % (rc, msg.decode() if msg else "?"))
        self._h = h
        with torch.cuda.device(self.device):
            shapes = param_shapes(self.F, self.H, self.C)
            self.params = [jl_empty(*s) for s in shapes]
            self.grads = [jl_zeros(*s) for s in shapes]
            self.mom = [jl_zeros(*s) for s in shapes]
            self.var = [jl_zeros(*s) for s in shapes]
        self.step = 0
        self.drop_seed = int(seed or 0)   # train_step's dropout draws step k with drop_seed + k
        self._opt_ctx = None
        self.use_stream(torch.cuda.current_stream(self.device))
        if seed is not None:
            self.init_weights(seed)

    # ---- plumbing
    def _call(self, name, *args):
        rc = getattr(_lib.lib(), name)(self._h, *args)
        if rc != 0:
            msg = _lib.lib().lrcn_act_last_error(self._h)
            raise LrcnError("%s error %d: %s" % (name, rc, msg.decode() if msg else "?"))

    def use_stream(self, stream):
        self._stream = stream
        self._call("lrcn_act_set_stream", C.c_void_p(stream.cuda_stream))

    def sync(self):
        self._stream.synchronize()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().lrcn_act_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _p4(ts):
        if len(ts) != 4 or any(t.dtype != torch.float32 for t in ts):
            raise LrcnError("an activity model is four float32 tensors (W, b, Wout, bout)")
        return _lib.P4(*[_ptr(t).value for t in ts])

    @staticmethod
    def _i32(a, n, what):
        if a is None:
            return None, None
        arr = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))
        if arr.size != n:
            raise LrcnError("%s has %d entries, expected %d" % (what, arr.size, n))
        return arr, arr.ctypes.data_as(C.POINTER(C.c_int32))

    def _feats(self, feats, B, T):
        if not torch.is_tensor(feats) or not feats.is_cuda:
            feats = to_jl(np.asarray(feats, np.float32))
        if tuple(feats.shape) != (B * T, self.F):
            raise LrcnError("feats must be (B*T) x F = %d x %d, got %s" % (B * T, self.F, tuple(feats.shape)))
        return feats

    # ---- model
    def init_weights(self, seed=1):
        self._call("lrcn_act_init_weights", self._p4(self.params), C.c_uint64(int(seed)))
        self.step = 0
        for t in self.mom + self.var:
            t.zero_()

    def _mask(self, mask, T, B, ncols, what):
        """A logical (T, B, ncols) multiplier array (numpy or device tensor) -> the ABI's T column-major blocks of B x ncols, on the device
        (lrcn._dropout's conversion)."""
        if mask is None:
            return None
        if torch.is_tensor(mask):
            m = mask.to(device="cuda:%d" % self.device, dtype=torch.float32)
        else:
            m = torch.as_tensor(np.asarray(mask, np.float32))
        if tuple(m.shape) != (T, B, ncols):
            raise LrcnError("%s must be (T, B, %d) = %s, got %s" % (what, ncols, (T, B, ncols), tuple(m.shape)))
        return m.permute(0, 2, 1).contiguous().to("cuda:%d" % self.device)

    def loss_grad(self, feats, labels, lens=None, T=None, grad=True, params=None, pdrop_in=0.0, pdrop_out=0.0, drop_seed=0, masks=None):
        """-> loss (float); grad=True also leaves d loss / d params in self.grads.  labels / lens: host int arrays [B] (lens None = T).
        pdrop_in / pdrop_out: seeded dropout on the frame features / on the LSTM output before the classifier (include/lrcn_act_dropout.h;
        the mask of a clip depends on its position in the batch and on B).  masks = (mask_in, mask_out): explicit multipliers in the
        logical shapes (T, B, F) / (T, B, H), either may be None; a mask replaces (p, seed) on its side.  With all four at their defaults
        the call is lrcn_act_loss_grad."""
        lab = np.asarray(labels, np.int32).reshape(-1)
        B = lab.size
        T = int(T if T is not None else self.max_T)
        feats = self._feats(feats, B, T)
        lab, plab = self._i32(lab, B, "labels")
        ln, plen = self._i32(lens, B, "lens")
        loss = C.c_double()
        g = self._p4(self.grads) if grad else None
        m_in, m_out = masks if masks is not None else (None, None)
        if not pdrop_in and not pdrop_out and m_in is None and m_out is None:
            self._call("lrcn_act_loss_grad", self._p4(params or self.params), _ptr(feats), plab, plen, T, B, g, C.byref(loss))
            return loss.value
        m_in, m_out = self._mask(m_in, T, B, self.F, "mask_in"), self._mask(m_out, T, B, self.H, "mask_out")
        d = _lib.ActDropout(float(pdrop_in or 0.0), float(pdrop_out or 0.0), int(drop_seed or 0) & (2 ** 64 - 1),
                            m_in.data_ptr() if m_in is not None else None, m_out.data_ptr() if m_out is not None else None)
        self._call("lrcn_act_loss_grad_drop", self._p4(params or self.params), _ptr(feats), plab, plen, T, B, C.byref(d), g, C.byref(loss))
        del m_in, m_out   # the device masks the struct points into: held until the call has returned (it synchronises for the loss)
        return loss.value

    def predict(self, feats, lens=None, T=None, B=None, frame_probs=False, params=None):
        """-> clip_probs (C x B column-major device tensor) [, frame_probs C x (B*T), column b*T + t]."""
        T = int(T if T is not None else self.max_T)
        if B is None:
            B = (lens.size if isinstance(lens, np.ndarray) else len(lens)) if lens is not None else feats.shape[0] // T
        feats = self._feats(feats, B, T)
        ln, plen = self._i32(lens, B, "lens")
        cp = jl_empty(self.C, B)
        fp = jl_empty(self.C, B * T) if frame_probs else None
        self._call("lrcn_act_predict", self._p4(params or self.params), _ptr(feats), plen, T, B, _ptr(cp), _ptr(fp) if fp is not None else None)
        return (cp, fp) if frame_probs else cp

    def _optimizer_ctx(self):
        if self._opt_ctx is None:
            from .lrcn import Context
            self._opt_ctx = Context(8, 8, 8, 8, max_B=1, max_T=1, device=self.device)
        return self._opt_ctx

    def adam_step(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, gclip=0.0):
        """update! with one Adam per tensor (lrcn_adam_update_flat, the caption path's arithmetic) from self.grads.  That entry point takes
        an lrcn_ctx: a minimal one (no VGG, a 8-unit caption shape) is made on first use and only ever runs this update.
        gclip > 0: the global gradient norm is clipped to it on the device (include/lrcn_clip.h): tensor k's sum of squares into slot k,
        lrcn_clip_set, then the clipped flat updates; self.grads keeps the unclipped gradient.  A model of more than nine tensors has no
        slot for its tenth: LrcnError."""
        ctx = self._optimizer_ctx()
        gclip = float(gclip or 0.0)
        self.step += 1
        L = _lib.lib()
        st = C.c_void_p(self._stream.cuda_stream)
        if gclip > 0:
            if len(self.grads) > 9:
                raise LrcnError("gradient-norm clipping has 9 slots, the model has %d tensors" % len(self.grads))
            for k, g in enumerate(self.grads):
                ctx._call("lrcn_grad_sumsq", C.c_void_p(g.data_ptr()), g.numel(), k, st)
            ctx._call("lrcn_clip_set", len(self.grads), gclip, st)
        update = L.lrcn_adam_update_flat_clipped if gclip > 0 else L.lrcn_adam_update_flat
        for p, g, m, v in zip(self.params, self.grads, self.mom, self.var):
            rc = update(ctx._h, C.c_void_p(p.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(m.data_ptr()),
                        C.c_void_p(v.data_ptr()), p.numel(), self.step, lr, beta1, beta2, eps, st)
            if rc != 0:
                raise LrcnError("lrcn_adam_update_flat error %d" % rc)

    def clip_stats(self):
        """The counters of adam_step(gclip > 0) (lrcn_clip_stats; waits for the model's stream)."""
        from . import lrcn
        self._stream.synchronize()
        return lrcn.clip_stats(self._optimizer_ctx())

    def train_step(self, feats, labels, lens=None, T=None, lr=1e-3, gclip=0.0, pdrop_in=0.0, pdrop_out=0.0):
        """loss_grad + adam_step.  pdrop_in / pdrop_out (the paper: 0.9 / 0.5): step k draws its masks with the seed drop_seed + k."""
        loss = self.loss_grad(feats, labels, lens, T, pdrop_in=pdrop_in, pdrop_out=pdrop_out, drop_seed=self.drop_seed + self.step)
        self.adam_step(lr, gclip=gclip)
        return loss

    def predict_videos(self, video_feats, T=None, stride=8, batch=None):
        """Per-video class distributions (C x n_videos, host) as the mean of their clips' and the per-clip (video, clip_probs [C]) list."""
        T = int(T if T is not None else self.max_T)
        batch = int(batch or self.max_B)
        specs = [(v, s, n) for v, f in enumerate(video_feats) for (s, n) in clips(f.shape[0], T, stride)]
        out = np.zeros((self.C, len(video_feats)), np.float64)
        cnt = np.zeros(len(video_feats))
        per_clip = []
        for i in range(0, len(specs), batch):
            sp = specs[i:i + batch]
            x, lens = gather_clips(video_feats, sp, T)
            cp = from_jl(self.predict(x, lens, T))
            for j, (v, _, _) in enumerate(sp):
                out[:, v] += cp[:, j]
                cnt[v] += 1
                per_clip.append((v, cp[:, j]))
        return out / np.maximum(cnt, 1), per_clip

    # ---- checkpoints
    def save(self, path):
        d = {"config": np.array([self.F, self.H, self.C, self.max_B, self.max_T, self.dtype, int(self.deterministic), self.step], np.int64),
             "drop_seed": np.array(self.drop_seed, np.int64)}
        for n, p, m, v in zip(PARAM_NAMES, self.params, self.mom, self.var):
            d[n] = from_jl(p)
            d["m_" + n] = from_jl(m)
            d["v_" + n] = from_jl(v)
        np.savez(path, **d)

    @classmethod
    def load(cls, path, max_B=None, max_T=None, dtype=None, device=None):
        z = np.load(path)
        F, H, C_, mb, mt, dt, det, step = [int(x) for x in z["config"]]
        self = cls(F, H, C_, max_B or mb, max_T or mt, dt if dtype is None else dtype, bool(det), device=device, seed=None)
        for i, n in enumerate(PARAM_NAMES):
            self.params[i].copy_(torch.as_tensor(z[n]))
            self.mom[i].copy_(torch.as_tensor(z["m_" + n]))
            self.var[i].copy_(torch.as_tensor(z["v_" + n]))
        self.step = step
        if "drop_seed" in z.files:   # checkpoints from before dropout have none: drop_seed stays 0
            self.drop_seed = int(z["drop_seed"])
        return self
