"""The sampler's fixture on both sides of the `stage` boundary (k_sample_rows keeps a logits row of up to 15360 columns in LDS), shared by
tests/test_sample_host.py (CPU) and tests/test_gpu_sample.py (GPU): a small f32 model whose LAST word holds a real share of every step's
distribution, and a free-running host sampler (the CPU oracle + tests/philox_ref.py) that shows the reference draws that word.  A staged copy
of the row that drops its last element cannot reproduce those draws."""
import functools

import numpy as np

import philox_ref as ph
from oracle import oracle as orc

STAGE_V = (15360, 15361)            # the last staged width and the first unstaged one
E = H = 16
N, S, NWORD = 3, 2, 4
SEED = 0x1234567890ABCDEF           # test_replay_small_f32's
DRAWS = ((1.0, 0), (1.0, 3))        # (temperature, top_k)
LAST_SHARE = (0.1, 0.5)             # p(V - 1) at every step of the host's own samples
EOS, BOS = 0, 1


@functools.lru_cache(maxsize=None)
def model(V):
    """test_gpu_sample.small_model at E = H = 16 with bout[V - 1] = log((V - 1) / 3): about a quarter of every row's mass."""
    m = orc.init_weights(E, H, H, V, seed=3)
    m.p["Wout"][:] *= 4.0
    m.p["bout"][0, V - 1] = np.float32(np.log((V - 1) / 3.0))
    return m


def feats():
    return (np.random.default_rng(7).standard_normal((N, 4096)) * 0.05).astype(np.float32)


@functools.lru_cache(maxsize=None)
def host_samples(V, T, top_k):
    """Free-running host samples of (image i, sample s): [(tokens incl. bos, [p(V - 1) of every step's row])], at most NWORD + 1 draws each
    (a caption ends at eos)."""
    m, f = model(V), feats()
    out = []
    for i in range(N):
        for s in range(S):
            seq, shares = [BOS], []
            for t in range(NWORD + 1):
                toks = np.zeros((max(t, 1), 1), np.int32)
                toks[:t, 0] = seq[1:t + 1]
                z = orc.forward_logits(m, f[i:i + 1], toks)[t, 0]
                shares.append(float(np.exp(ph.log_softmax(z)[V - 1])))
                seq.append(int(ph.draw(z, T, top_k, SEED, i, s, t + 1)))
                if seq[-1] == EOS:
                    break
            out.append((seq, shares))
    return out
