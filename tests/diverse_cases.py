"""The small-model cases that tests/test_gpu_diverse.py holds against tests/diverse_ref.py, shared with tests/test_diverse_host.py, which
checks on the host alone that the reference's answers on these inputs do not hang on the last bits of the logits."""
import numpy as np

from oracle import oracle as orc

ES, VS, NWORD = 64, 203, 12
LAYERS = (2, 1)
KG = ((4, 2), (6, 3), (8, 8), (10, 5), (32, 4), (32, 32))
LAMBDAS = (0.5, 2.0)
ALPHAS = (0.0, 1.0)
FEAT_SEED = {}   # (n_layers, K, G, lambda, alpha) -> seed of the features, where the default's answers were not stable
DEFAULT_FEAT_SEED = 7


def cases():
    return [(nl, K, G, lam, alpha) for nl in LAYERS for K, G in KG for lam in LAMBDAS for alpha in ALPHAS]


def n_images(K):
    return 4 if K == 32 else 8


def small_model(n_layers=2, seed=3, spread=16.0):
    """as test_gpu_nbest.py's: spread in the word distributions, still far from peaky"""
    m = orc.init_weights(ES, ES, ES, VS, seed=seed, n_layers=n_layers)
    m.p["Wout"][:] *= spread
    return m


def feats_of(N, seed):
    return (np.random.default_rng(seed).standard_normal((N, 4096)) * 0.05).astype(np.float32)


def case_inputs(case):
    nl, K, _, _, _ = case
    return small_model(n_layers=nl), feats_of(n_images(K), FEAT_SEED.get(case, DEFAULT_FEAT_SEED))
