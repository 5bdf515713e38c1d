"""Host measures of how diverse a list of captions is (for n-best and diverse beam lists; include/lrcn_diverse.h).  Captions are token
lists (ids or words); callers strip bos / eos as they see fit."""


def _ngrams(tokens, n):
    return [tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1)]


def distinct_n(captions, n):
    """Distinct n-grams over all n-grams of the list (Li et al. 2016): 1.0 = no n-gram repeats, 0.0 for a list without n-grams."""
    grams = [g for c in captions for g in _ngrams(list(c), n)]
    return len(set(grams)) / len(grams) if grams else 0.0


def mean_pairwise_overlap(captions, n=1):
    """Mean over the unordered pairs of captions of |A & B| / |A | B|, A and B the captions' sets of n-grams (a pair without n-grams counts
    as 1.0: two empty captions are the same caption); 0.0 for fewer than two captions.  1.0 = every pair shares all its n-grams."""
    sets = [set(_ngrams(list(c), n)) for c in captions]
    tot, pairs = 0.0, 0
    for i in range(len(sets)):
        for j in range(i + 1, len(sets)):
            u = sets[i] | sets[j]
            tot += len(sets[i] & sets[j]) / len(u) if u else 1.0
            pairs += 1
    return tot / pairs if pairs else 0.0
