"""Caption evaluation: CIDEr-D (Vedantam, Zitnick and Parikh 2015, "CIDEr: Consensus-based Image Description Evaluation", as the COCO
caption evaluation computes it) -- the reward of self-critical training (scst.py) and a metric with a length term, which bleu.py's
restatement of the reference's script (brevity penalty off) is not.  Host-only code.

The fixed choices:
  n-grams           n = 1..4 of the word sequence (whitespace tokens; the caller lower-cases and strips punctuation as it wants)
  document          one per image: the union of its references' n-grams; df(g) = the number of images whose references contain g
  idf(g)            log(N / max(1, df(g))), N = the number of images
  vector            per n, v[g] = count(g) * idf(g); |v| = its Euclidean norm
  similarity        per n, sum_g min(v_h[g], v_r[g]) * v_r[g] / (|v_h| |v_r|)   (the hypothesis counts clipped to the reference's; 0 when a
                    norm is 0), times the length penalty exp(-(l_h - l_r)^2 / (2 sigma^2)), sigma = 6, l = the number of words
  score             the mean over the image's references, then over n = 1..4, times 10
An empty hypothesis scores 0.
"""
import math
from collections import Counter

N_MAX = 4
SIGMA = 6.0


def _words(caption):
    return caption.split() if isinstance(caption, str) else list(caption)


def _counts(words):
    """One Counter per n = 1..4."""
    return [Counter(tuple(words[i:i + n]) for i in range(len(words) - n + 1)) for n in range(1, N_MAX + 1)]


class CiderD:
    def __init__(self, refs_by_image):
        """refs_by_image: {image_id: [reference, ...]}, a reference being a list of words or a string."""
        self.n_images = len(refs_by_image)
        if self.n_images == 0:
            raise ValueError("CiderD needs at least one image's references")
        counts = {i: [(_counts(_words(r)), len(_words(r))) for r in refs] for i, refs in refs_by_image.items()}
        df = [Counter() for _ in range(N_MAX)]
        for refs in counts.values():
            for n in range(N_MAX):
                df[n].update(set().union(*[c[n].keys() for c, _ in refs]) if refs else ())
        log_n = math.log(self.n_images)
        self._idf = [{g: log_n - math.log(max(1, d)) for g, d in df[n].items()} for n in range(N_MAX)]
        self._log_n = log_n
        self._refs = {i: [self._vectors(c) + (length,) for c, length in refs] for i, refs in counts.items()}

    def idf(self, ngram):
        """idf of an n-gram (a tuple of words); an n-gram in no reference counts as df = 0 -> log N."""
        return self._idf[len(ngram) - 1].get(tuple(ngram), self._log_n)

    def _vectors(self, counts):
        vecs, norms = [], []
        for n in range(N_MAX):
            idf = self._idf[n]
            v = {g: c * idf.get(g, self._log_n) for g, c in counts[n].items()}
            vecs.append(v)
            norms.append(math.sqrt(sum(x * x for x in v.values())))
        return vecs, norms

    def score(self, image_id, words):
        """CIDEr-D of one hypothesis (list of words or string) against image_id's references."""
        words = _words(words)
        refs = self._refs[image_id]
        if not words or not refs:
            return 0.0
        hv, hn = self._vectors(_counts(words))
        total = 0.0
        for rv, rn, rlen in refs:
            pen = math.exp(-float(len(words) - rlen) ** 2 / (2.0 * SIGMA * SIGMA))
            for n in range(N_MAX):
                if hn[n] == 0.0 or rn[n] == 0.0:
                    continue
                dot = sum(min(x, rv[n][g]) * rv[n][g] for g, x in hv[n].items() if g in rv[n])
                total += pen * dot / (hn[n] * rn[n])
        return 10.0 * total / (N_MAX * len(refs))

    def corpus(self, hyps_by_image):
        """{image_id: hypothesis} -> (mean, {image_id: score})."""
        per = {i: self.score(i, h) for i, h in hyps_by_image.items()}
        return (sum(per.values()) / len(per) if per else 0.0), per
