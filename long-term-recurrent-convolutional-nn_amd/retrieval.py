"""Image-caption retrieval metrics (paper section 5.1 / Table 2; not in lrcn.jl): R@1, R@5, R@10 and Medr in both directions from a score
matrix s(n, m) = log p(caption m | image n) -- lrcn.score_matrix.  Pure numpy."""
import numpy as np

KS = (1, 5, 10)


def _ranks_desc(v):
    """1-based rank of every entry of v under a stable descending order (a tie goes to the lower index)."""
    order = np.argsort(-np.asarray(v, np.float64), kind="stable")
    rk = np.empty(len(order), np.int64)
    rk[order] = np.arange(1, len(order) + 1)
    return rk


def metrics(scores, img_of_caption, norm="mean", lens=None):
    """scores N x M (image n, caption m), img_of_caption [M]: the ground-truth image of every caption.

    Caption to image: caption m ranks the N images by s(n, m); its rank is that of its image.  Image to caption: image n ranks the M captions;
    its rank is the best rank among its ground-truth captions.  R@K = percentage of queries with rank <= K; Medr = numpy.median of the ranks.
    Ties: stable descending order, so the lower index wins (as in the beam's ranking).
    norm "sum": the scores as given; "mean": each caption's score divided by (L_m + 1), its number of predicted tokens (lens [M] = L_m
    required).  A caption-to-image ranking compares one caption's scores only, so it does not depend on the normalisation.
    Returns {"caption_to_image": {"R@1", "R@5", "R@10", "Medr"}, "image_to_caption": {...}}."""
    s = np.asarray(scores, np.float64)
    if s.ndim != 2:
        raise ValueError("scores must be N x M")
    N, M = s.shape
    gt = np.asarray(img_of_caption, np.int64)
    if gt.shape != (M,) or (M and (gt.min() < 0 or gt.max() >= N)):
        raise ValueError("img_of_caption must hold M image indices in [0, N)")
    if norm == "mean":
        if lens is None:
            raise ValueError('norm="mean" needs the caption lengths')
        L = np.asarray(lens, np.float64)
        if L.shape != (M,):
            raise ValueError("lens must have M entries")
        s = s / (L + 1.0)[None, :]
    elif norm != "sum":
        raise ValueError('norm must be "mean" or "sum"')
    c2i = np.array([_ranks_desc(s[:, m])[gt[m]] for m in range(M)], np.int64)
    i2c = []
    for n in range(N):
        caps = np.nonzero(gt == n)[0]
        if len(caps) == 0:
            continue   # an image without a ground-truth caption is not a query
        i2c.append(_ranks_desc(s[n, :])[caps].min())
    i2c = np.array(i2c, np.int64)

    def summary(r):
        out = {"R@%d" % k: float(100.0 * np.mean(r <= k)) for k in KS}
        out["Medr"] = float(np.median(r))
        return out

    return {"caption_to_image": summary(c2i), "image_to_caption": summary(i2c)}


def format_line(name, m):
    """'Caption to Image: R@1 40.0 R@5 ... Medr 2.0'"""
    return "%s: R@1 %.1f R@5 %.1f R@10 %.1f Medr %.1f" % (name, m["R@1"], m["R@5"], m["R@10"], m["Medr"])
