"""CIDEr-D on the device (include/lrcn_cider.h): cider.CiderD's metric over token ids, scored by one HIP kernel call per batch of captions
instead of a Python loop per caption -- the reward of self-critical training (scst.scst_step(reward=DeviceCiderD(...))) and the per-epoch
dev metric (scst.beam_cider).

The references are turned into ids once, with `word_to_index`; a word outside it becomes `unk_index`.  Hypotheses are ids from the start:
the sampler's and the beam search's own output.  The scores equal cider.CiderD's on the corresponding WORDS exactly when
  * the host metric's references were unk-mapped the same way -- scst.references_by_image(caps, vocab), what tools/lrcn.py does -- and
  * the id -> word table the host reward uses is one to one (two ids that print as the same word are two words here),
and then to a few units of rounding (the sums run in another order; tests/test_gpu_cider.py holds them to 1e-12).  There is no host path
in this module: without the library and a GPU it raises."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import LrcnError

MAX_WORDS = 256   # LRCN_CIDER_MAXWORDS


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class DeviceCiderD:
    def __init__(self, refs_by_image, word_to_index, unk_index, device=None):
        """refs_by_image: {image_id: [reference, ...]} as cider.CiderD takes it (a reference: a list of words or a string);
        word_to_index: word -> id in [0, V); words outside it count as id unk_index.  V = the largest id + 1."""
        if not torch.cuda.is_available():
            raise LrcnError("no MI355X visible: liblrcn_hip has no CPU path")
        if len(refs_by_image) == 0:
            raise ValueError("DeviceCiderD needs at least one image's references")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.index_of = {image_id: k for k, image_id in enumerate(refs_by_image)}
        self.V = max(max(word_to_index.values(), default=0), int(unk_index)) + 1
        unk = int(unk_index)
        ref_image, offsets, toks = [], [0], []
        for image_id, refs in refs_by_image.items():
            for r in refs:
                words = r.split() if isinstance(r, str) else list(r)
                toks.extend(word_to_index.get(w, unk) for w in words)
                offsets.append(len(toks))
                ref_image.append(self.index_of[image_id])
        ref_image, toks = _i32(ref_image), _i32(toks)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        h = C.c_void_p()
        rc = _lib.lib().lrcn_cider_create(self.device, len(self.index_of), len(ref_image), _ptr(ref_image, C.c_int32), _ptr(offsets, C.c_int64),
                                          _ptr(toks, C.c_int32), self.V, C.byref(h))
        if rc != 0:
            msg = _lib.lib().lrcn_cider_last_error(None)
            raise LrcnError("lrcn_cider_create error %d: %s" % (rc, msg.decode() if msg else "?"))
        self._h = h
        self.use_stream(torch.cuda.current_stream(self.device))

    # ---- plumbing
    def _call(self, name, *args):
        rc = getattr(_lib.lib(), name)(self._h, *args)
        if rc != 0:
            msg = _lib.lib().lrcn_cider_last_error(self._h)
            raise LrcnError("%s error %d: %s" % (name, rc, msg.decode() if msg else "?"))

    def use_stream(self, stream):
        self._stream = stream
        self._call("lrcn_cider_set_stream", C.c_void_p(stream.cuda_stream))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().lrcn_cider_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        """-> {"images", "references", "ngrams" [4], "slots" [4], "ref_entries" [4], "device_bytes"} (lrcn_cider_stats_t)."""
        s = _lib.CiderStats()
        self._call("lrcn_cider_stats", C.byref(s))
        return {"images": int(s.images), "references": int(s.references), "ngrams": [int(x) for x in s.ngrams], "slots": [int(x) for x in s.slots],
                "ref_entries": [int(x) for x in s.ref_entries], "device_bytes": int(s.device_bytes)}

    def _indices(self, image_ids):
        try:
            return _i32([self.index_of[i] for i in image_ids])
        except KeyError as e:
            raise LrcnError("image %r has no references in this DeviceCiderD" % (e.args[0],))

    # ---- scoring
    def score_rows(self, image_index, tokens, out_len):
        """lrcn_cider_score as it is: image_index [R] int32 (indices, not ids), tokens [R][ld], out_len [R] -> float64 [R]."""
        tokens, out_len, image_index = _i32(tokens), _i32(out_len), _i32(image_index)
        if tokens.ndim != 2 or out_len.shape != (tokens.shape[0],) or image_index.shape != out_len.shape:
            raise LrcnError("score_rows wants image_index [R], tokens [R][ld] and out_len [R]")
        out = np.empty(tokens.shape[0], np.float64)
        self._call("lrcn_cider_score", _ptr(tokens, C.c_int32), int(tokens.shape[1]), _ptr(out_len, C.c_int32), _ptr(image_index, C.c_int32),
                   int(tokens.shape[0]), _ptr(out, C.c_double))
        return out

    def score_ids(self, image_ids, tokens, out_len):
        """The sampler's arrays as they are: tokens [R][ld] int32 (bos first), out_len [R] (counting bos and a closing eos), image_ids [R]
        -> float64 [R].  One call: copies in, one kernel, copies out."""
        return self.score_rows(self._indices(image_ids), tokens, out_len)

    def score_rows_dev(self, image_index, tokens, out_len, out=None):
        """lrcn_cider_score_dev: int32 device tensors image_index [R], tokens [R][ld] (contiguous), out_len [R] -> float64 device tensor
        [R], queued on the handle's stream without a synchronise.  The rows are the caller's contract (include/lrcn_cider.h)."""
        for t in (image_index, tokens, out_len):
            if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
                raise LrcnError("score_rows_dev wants contiguous int32 device tensors")
        R, ld = int(tokens.shape[0]), int(tokens.shape[1])
        if tokens.dim() != 2 or tuple(out_len.shape) != (R,) or tuple(image_index.shape) != (R,):
            raise LrcnError("score_rows_dev wants image_index [R], tokens [R][ld] and out_len [R]")
        if out is None:
            out = torch.empty(R, dtype=torch.float64, device=tokens.device)
        self._call("lrcn_cider_score_dev", C.c_void_p(tokens.data_ptr()), ld, C.c_void_p(out_len.data_ptr()), C.c_void_p(image_index.data_ptr()), R,
                   C.c_void_p(out.data_ptr()))
        return out

    def score_batch(self, image_ids, id_lists):
        """image_ids [R] and R lists of word ids (no bos, no eos; at most 256 each) -> float64 [R], in one call."""
        R = len(id_lists)
        if len(image_ids) != R:
            raise LrcnError("%d image ids for %d captions" % (len(image_ids), R))
        if R == 0:
            return np.zeros(0, np.float64)
        n = np.asarray([len(w) for w in id_lists], np.int32)
        tok = np.full((R, int(n.max()) + 2), _lib.EOS, np.int32)
        tok[:, 0] = _lib.BOS
        for r, w in enumerate(id_lists):
            tok[r, 1:1 + len(w)] = w
        return self.score_ids(image_ids, tok, n + 2)   # every row closes with eos

    def score(self, image_id, ids):
        """One caption's score (cider.CiderD.score on ids)."""
        return float(self.score_batch([image_id], [ids])[0])

    def corpus(self, hyps_by_image):
        """{image_id: word ids} -> (mean, {image_id: score}), shaped like cider.CiderD.corpus."""
        ids = list(hyps_by_image)
        s = self.score_batch(ids, [hyps_by_image[i] for i in ids])
        per = {i: float(x) for i, x in zip(ids, s)}
        return (sum(per.values()) / len(per) if per else 0.0), per
