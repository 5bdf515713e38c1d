"""CPU: lrcn_amd/cider.py (CIDEr-D) on a corpus small enough to work by hand.  No GPU, no HIP library.

The corpus: N = 3 images, two references each.
    A: "a dog runs"      "the dog runs fast"
    B: "a cat sleeps"    "the cat sleeps now"
    C: "a bird sings"    "the bird sings loudly"
Document frequencies are per image: "a" and "the" are in all three -> idf = log(3 / 3) = 0; every other n-gram of the references is in one
image only -> idf = l := log 3 (an n-gram in no reference: df = 0 -> log(3 / max(1, 0)) = l as well).  A tf-idf vector's entry is
count * idf, so with one occurrence each the entries are 0 or l and cosines come out as ratios of square roots.
score = 10 * mean over the two references, mean over n = 1..4, of  cosine_n * exp(-(l_h - l_r)^2 / 72)   (sigma = 6: 2 sigma^2 = 72)."""
import math

import pytest

from lrcn_amd.cider import CiderD

REFS = {"A": ["a dog runs", "the dog runs fast"],
        "B": ["a cat sleeps".split(), "the cat sleeps now".split()],     # word lists and strings are both accepted
        "C": ["a bird sings", "the bird sings loudly"]}
s2, s3, s6 = math.sqrt(2), math.sqrt(3), math.sqrt(6)


def pen(d):
    return math.exp(-d * d / 72.0)


@pytest.fixture(scope="module")
def cider():
    return CiderD(REFS)


def test_idf_of_an_ngram_in_every_image_is_zero(cider):
    assert cider.idf(("a",)) == 0.0 and cider.idf(("the",)) == 0.0
    assert abs(cider.idf(("dog",)) - math.log(3)) < 1e-15 and abs(cider.idf(("dog", "runs")) - math.log(3)) < 1e-15
    assert abs(cider.idf(("zebra",)) - math.log(3)) < 1e-15
    # "a the": the unigram vector is all zeros (norm 0 -> similarity 0), the bigram (a, the) is in no reference
    assert cider.score("A", "a the") == 0.0


def test_a_hypothesis_equal_to_a_reference(cider):
    # h = "a dog runs" against A.
    # vs "a dog runs" (identical, penalty 1): n = 1, 2, 3 cosine 1; n = 4: h has no 4-gram -> 0.                 sum = 3
    # vs "the dog runs fast" (l_r = 4, penalty pen(1)):
    #   n = 1: h = {a: 0, dog: l, runs: l}, r = {the: 0, dog: l, runs: l, fast: l}; dot = 2 l^2, |h| = l sqrt 2, |r| = l sqrt 3 -> 2 / sqrt 6
    #   n = 2: h = {(a dog), (dog runs)}, r = {(the dog), (dog runs), (runs fast)}, all l; dot = l^2                    -> 1 / sqrt 6
    #   n = 3: no common trigram -> 0;  n = 4: 0                                                                  sum = 3 / sqrt 6
    want = 10.0 * (3.0 + pen(1) * 3.0 / s6) / 8.0
    got = cider.score("A", "a dog runs")
    assert abs(got - want) < 1e-12, (got, want)
    assert abs(cider.score("A", ["a", "dog", "runs"]) - want) < 1e-12
    # a word swapped: "a dog sleeps" keeps dog (n = 1) and (a dog) (n = 2) only
    #   vs ref 1: n = 1: dot l^2 / (l sqrt 2 * l sqrt 2) = 1/2; n = 2: {(a dog), (dog sleeps)} . {(a dog), (dog runs)} = 1/2; n = 3: 0
    #   vs ref 2: n = 1: l^2 / (l sqrt 2 * l sqrt 3) = 1 / sqrt 6; n = 2: no common bigram
    swapped = cider.score("A", "a dog sleeps")
    assert abs(swapped - 10.0 * (1.0 + pen(1) / s6) / 8.0) < 1e-12
    assert swapped < got


def test_word_order_matters_from_n_2(cider):
    # "runs dog a" has the unigrams of "a dog runs" and none of its bigrams or trigrams (its own are in no reference: dot 0)
    #   vs ref 1: n = 1: 1;  vs ref 2: n = 1: 2 / sqrt 6 with pen(1)
    got = cider.score("A", "runs dog a")
    assert abs(got - 10.0 * (1.0 + pen(1) * 2.0 / s6) / 8.0) < 1e-12
    assert got < cider.score("A", "a dog runs")


def test_a_much_longer_hypothesis_is_penalised(cider):
    # "dog": n = 1 only.  vs ref 1 (l_r = 3): l^2 / (l * l sqrt 2) = 1 / sqrt 2, pen(2); vs ref 2 (l_r = 4): 1 / sqrt 3, pen(3)
    short = cider.score("A", "dog")
    assert abs(short - 10.0 * (pen(2) / s2 + pen(3) / s3) / 8.0) < 1e-12
    # "dog the the the the the the the the the the the" (12 words): "the" has idf 0, so the unigram vector and both cosines are the
    # same; its bigrams (dog the), (the the) are in no reference.  Only the penalties change: pen(9), pen(8)
    long = cider.score("A", "dog" + " the" * 11)
    assert abs(long - 10.0 * (pen(9) / s2 + pen(8) / s3) / 8.0) < 1e-12
    assert long < 0.5 * short


def test_hypothesis_counts_are_clipped_to_the_references(cider):
    # "dog dog": n = 1: h = {dog: 2 l}; vs ref 1: min(2 l, l) * l = l^2 over (2 l)(l sqrt 2) = 1 / (2 sqrt 2), pen(1);
    # vs ref 2: 1 / (2 sqrt 3), pen(2).  n = 2: (dog dog) is in no reference.  (Unclipped, the dot would be 2 l^2: twice as much.)
    got = cider.score("A", "dog dog")
    assert abs(got - 10.0 * (pen(1) / (2 * s2) + pen(2) / (2 * s3)) / 8.0) < 1e-12


def test_an_empty_hypothesis_scores_zero_and_corpus_is_the_mean_of_score(cider):
    assert cider.score("A", "") == 0.0 and cider.score("B", []) == 0.0
    hyps = {"A": "a dog runs", "B": "the cat sleeps now", "C": ""}
    mean, per = cider.corpus(hyps)
    assert set(per) == set(hyps) and per["C"] == 0.0
    for k, h in hyps.items():
        assert per[k] == cider.score(k, h)
    assert abs(mean - sum(per.values()) / 3.0) < 1e-15
    # by the symmetry of the corpus, B's second reference scores as A's would: identical vs ref 2 (n = 1..4 all 1), and vs ref 1
    # "a cat sleeps" the 2 / sqrt 6 + 1 / sqrt 6 of above with pen(1)
    assert abs(per["B"] - 10.0 * (4.0 + pen(1) * 3.0 / s6) / 8.0) < 1e-12
    with pytest.raises(ValueError):
        CiderD({})
