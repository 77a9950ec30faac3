"""TEST INFRASTRUCTURE -- the definition of sampled generation (include/tst_hip.h tst_sample_async), with no cache and no device: Philox4x32-10 in numpy, the
Gumbel noise g = -log(-log u) in float64 from the same u = ((x >> 9) + 0.5) 2^-23, and `sampled`, which re-runs the pinned oracle's forward_logits on the growing
sequences and takes argmax(logits / temperature + g) (first index of the maximum). Built on tests/generate_oracle.py; every reference is computed once per
process and kept.

A draw is DECIDABLE when the gap between its largest and second largest perturbed score exceeds
    band(temperature) = 2 LOGIT_TOL / temperature + 2e-5
LOGIT_TOL = 1e-4 is tests/test_strict_gpu.py's bound on one strict logit (two logits may move against each other); 2e-5 covers the device's fp32 noise and fp32
score sum: |g| <= 16.7 whose fp32 ulp is 1.9e-6 -- about four ulp for the two logarithms, and one rounding of a score of up to 64 on either side.

SAMPLE_SEED: per (family, adapter, temperature) case the first `sample_seed` (searched on the CPU, tests/test_sample_cpu.py pins it) for which no draw of the
oracle's trajectory has a gap under 2 band: on random logits about 0.05 % of draws fall under 1e-3, so a 288-draw case misses the condition now and then."""
import functools

import numpy as np

import generate_oracle as G

LOGIT_TOL = 1e-4   # tests/test_strict_gpu.py
N_SAMPLES = 4
TEMPERATURES = (1.0, 0.5)
ADAPTERS = (None, 99)

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def band(temperature):
    return 2 * LOGIT_TOL / temperature + 2e-5


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (k0, k1) of 32-bit words -> the four output words [..., 4] uint32 (Salmon et al., SC'11; ten rounds)"""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) & _MASK for i in range(4)]
    k0, k1 = (np.asarray(key)[..., i].astype(np.uint64) & _MASK for i in range(2))
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def uniform_of(x):
    """u = ((x >> 9) + 0.5) 2^-23 in float64: 24 significant bits, exact in fp32 too, never 0 or 1"""
    return ((np.asarray(x, np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def noise_words(seed, V, step, sample):
    """the 32-bit word of every vocabulary entry v < V: word v & 3 of counter (v >> 2, step, sample, 0) under key (low, high 32 bits of seed)"""
    nq = (V + 3) // 4
    ctr = np.zeros((nq, 4), np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2] = np.arange(nq), step, sample
    seed = int(seed)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64)
    return philox4x32_10(ctr, key).reshape(-1)[:V]


def gumbel(seed, V, step, sample):
    """g [V] float64"""
    return -np.log(-np.log(uniform_of(noise_words(seed, V, step, sample))))


def draw(logits, temperature, g):
    """one draw from rows of logits [..., V] with noise g of the same shape: (token, log softmax(logits / temperature)[token], top-1 / top-2 gap of the scores)"""
    z = np.asarray(logits, np.float64) / temperature
    sc = z + g
    tok = sc.argmax(-1)
    top2 = np.partition(sc, -2, axis=-1)[..., -2:]
    gap = top2[..., 1] - top2[..., 0]
    logp = np.take_along_axis(G.log_softmax(z), tok[..., None], -1)[..., 0]
    return tok.astype(np.int32), logp, gap


def sampled(orc, prompts, n, temperature, seeds, max_new=G.MAX_NEW):
    """tokens [S, n, max_new] int32, logp (same, float64), gap (same): n draws per prompt, max_new forwards of the oracle over the growing sequences (step 0 over
    the S prompts, whose last-row logits all n samples of a prompt read)"""
    S = len(prompts)
    V = None
    seqs = [[list(map(int, p)) for _ in range(n)] for p in prompts]
    tokens, logp, gap = np.zeros((S, n, max_new), np.int32), np.zeros((S, n, max_new)), np.zeros((S, n, max_new))
    for j in range(max_new):
        if j == 0:
            ids, cu = G.pack([p for p in prompts])
            lg = np.asarray(orc.forward_logits(ids, cu, cu[1:] - 1), np.float64)
            lg = np.repeat(lg[:, None], n, 1)
        else:
            ids, cu = G.pack([q for row in seqs for q in row])
            lg = np.asarray(orc.forward_logits(ids, cu, cu[1:] - 1), np.float64).reshape(S, n, -1)
        V = lg.shape[-1]
        g = np.stack([np.stack([gumbel(seeds[s], V, j, i) for i in range(n)]) for s in range(S)])
        tokens[:, :, j], logp[:, :, j], gap[:, :, j] = draw(lg, temperature, g)
        for s in range(S):
            for i in range(n):
                seqs[s][i].append(int(tokens[s, i, j]))
    return tokens, logp, gap


def prompt_seeds(sample_seed, n):
    from tst.score import sample_seeds
    return sample_seeds(sample_seed, np.arange(n))


# (family, adapter seed, temperature) -> sample_seed: the first seed 0, 1, ... whose trajectory has no draw with a gap under 2 band (tests/test_sample_cpu.py
# pins it); the cases not listed pass with seed 0
SAMPLE_SEED = {("tiny", 99, 0.5): 1, ("tiny2", 99, 1.0): 1, ("gpt2", 99, 0.5): 1, ("qwen3", None, 0.5): 1}


def case_seed(tag, lora_seed, temperature):
    return SAMPLE_SEED.get((tag, lora_seed, temperature), 0)


@functools.lru_cache(maxsize=None)
def sampled_reference(tag, lora_seed=None, temperature=1.0, sample_seed=None):
    """the fp32 oracle's sampled continuations of the shared prompts of a family: (tokens, logp, gap, seeds)"""
    prompts = G.make_prompts(G.FAMILIES[tag])
    seeds = prompt_seeds(case_seed(tag, lora_seed, temperature) if sample_seed is None else sample_seed, len(prompts))
    return sampled(G.make_oracle(tag, lora_seed), prompts, N_SAMPLES, temperature, seeds) + (seeds,)


def replay_rows(prompts, tokens):
    """the S * n sampled sequences packed, s-major, and the rows whose logits chose each drawn token: (ids, cu, rows [S * n * max_new])"""
    S, n, _ = tokens.shape
    return G.replay_rows([prompts[s] for s in range(S) for _ in range(n)], tokens.reshape(S * n, -1))


# ---- coverage: the first tokens of COVER_SEEDS x COVER_N draws of ONE prompt against softmax(O / temperature)
COVER_SEEDS, COVER_N, COVER_PROMPT, COVER_SAMPLE_SEED = 8, 64, 2, 11


def cover_seeds():
    return prompt_seeds(COVER_SAMPLE_SEED, COVER_SEEDS)


def first_token_chi2(counts_by_token, probs, n_draws):
    """chi-square of first-token counts against probs over the eight likeliest tokens + the rest (8 degrees of freedom: 43.3 is p = 1e-6)"""
    top = np.argsort(-probs, kind="stable")[:8]
    obs = np.array([counts_by_token[t] for t in top] + [n_draws - sum(counts_by_token[t] for t in top)], np.float64)
    exp = np.concatenate([probs[top], [1.0 - probs[top].sum()]]) * n_draws
    return float(((obs - exp) ** 2 / exp).sum())
