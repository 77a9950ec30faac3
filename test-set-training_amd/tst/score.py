"""Per-sample bias score s(x) from the per-row quantities tst_score returns (the upstream README
only names s(x), so the definition is this build's and is frozen here):

  * multiple-choice sample (answer = one option-letter token): softmax over the option-letter logits at the answer
    position; s(x) = p[ground truth], prediction = argmax over the options.
  * numeric / open answer (1..4 tokens): s(x) = exp(mean_t log p(answer_t | prefix)), teacher-forced;
    correct iff every answer token is the arg-max token.

With attribution switched on (TrainArgs.attribute) a sample also carries WHICH prompt tokens its score rests on: the gradient of log s(x) with respect to every
prompt token's embedding output, as gradient x input and as gradient norm (token_attribution; the definition is frozen in include/tst_hip.h
tst_attribute_async). log s is differentiated rather than s so that the scale does not collapse for confident samples; d s = s d log s.
With integrated gradients (token_ig; tst_attribute_ig_async) the prompt tokens instead share out, with sign, the change of log s(x) between a prompt of baseline
tokens and the real one.

With generation switched on (TrainArgs.generate) a sample also carries what the text-only model SAYS: its greedy continuation of the prompt
(generated_answers), and gen_correct = that continuation starts with the reference answer's tokens. bias_scores does not change.
"""
import numpy as np


def bias_scores(samples, logp, correct_rows, opt_logits, row_seq):
    """samples: the held-out samples of the scored batch, in batch order; row arrays as returned by Context.score_rows.
    Returns (s[n], pred[n], correct[n]) with pred = option index for MCA samples and -1 otherwise."""
    n = len(samples)
    s = np.zeros(n, np.float32)
    pred = np.full(n, -1, np.int32)
    correct = np.zeros(n, np.int32)
    row_seq = np.asarray(row_seq)
    for i, smp in enumerate(samples):
        rows = np.flatnonzero(row_seq == i)
        if len(rows) != smp.n_answer:
            raise ValueError(f"sample {smp.sid}: expected {smp.n_answer} answer rows, got {len(rows)}")
        if smp.kind == "mca":
            z = opt_logits[rows[0]].astype(np.float64)
            p = np.exp(z - z.max())
            p /= p.sum()
            s[i] = p[smp.gt_option]
            pred[i] = int(np.argmax(z))
            correct[i] = int(pred[i] == smp.gt_option)
        else:
            s[i] = np.exp(np.mean(logp[rows].astype(np.float64)))
            correct[i] = int(correct_rows[rows].all())
    return s, pred, correct


def attribution_kinds(samples):
    """seq_kind of Context.attribute for the samples of a batch: 1 (option form) for multiple-choice samples, 0 (open form) otherwise"""
    return np.array([1 if s.kind == "mca" else 0 for s in samples], np.int32)


def token_attribution(samples, gxi, gnorm, logs):
    """samples: the attributed batch in batch order (full sequences, as data.collate packs them); gxi / gnorm per token and logs per sample as returned by
    Context.attribute. Returns per sample dict(gxi, gnorm: the prompt tokens' values, share: gnorm / sum of gnorm over the prompt, log_s)."""
    gxi, gnorm = np.asarray(gxi, np.float32), np.asarray(gnorm, np.float32)
    if len(gxi) != sum(len(s.ids) for s in samples) or len(gnorm) != len(gxi) or len(logs) != len(samples):
        raise ValueError("token_attribution: the arrays do not belong to this batch")
    out, o = [], 0
    for i, smp in enumerate(samples):
        g, n = gxi[o:o + smp.n_prompt].copy(), gnorm[o:o + smp.n_prompt].copy()
        tot = float(n.astype(np.float64).sum())
        out.append(dict(gxi=g, gnorm=n, share=(n / tot if tot > 0 else np.zeros_like(n)).astype(np.float32), log_s=float(logs[i])))
        o += len(smp.ids)
    return out


def ig_baseline_ids(samples, baseline_id):
    """baseline_ids of Context.attribute_ig for the samples of a batch (full sequences, in batch order): baseline_id on every prompt token, the token's own id
    on the answer tokens -- those are not interpolated, so the teacher-forced answer stays what it is"""
    out = []
    for smp in samples:
        row = np.asarray(smp.ids, np.int32).copy()
        row[:smp.n_prompt] = baseline_id
        out.append(row)
    return np.concatenate(out) if out else np.zeros(0, np.int32)


def token_ig(samples, ig, logs, logs_base):
    """samples: the attributed batch in batch order (full sequences, as data.collate packs them); ig per token, logs / logs_base per sample as returned by
    Context.attribute_ig. Returns per sample dict(ig: the prompt tokens' values, log_s, log_s_base, delta = sum of ig over ALL tokens of the sample
    - (log_s - log_s_base): the completeness gap, 0 in the limit of many steps)."""
    ig = np.asarray(ig, np.float32)
    if len(ig) != sum(len(s.ids) for s in samples) or len(logs) != len(samples) or len(logs_base) != len(samples):
        raise ValueError("token_ig: the arrays do not belong to this batch")
    out, o = [], 0
    for i, smp in enumerate(samples):
        n = len(smp.ids)
        total = float(ig[o:o + n].astype(np.float64).sum())
        out.append(dict(ig=ig[o:o + smp.n_prompt].copy(), log_s=float(logs[i]), log_s_base=float(logs_base[i]),
                        delta=total - (float(logs[i]) - float(logs_base[i]))))
        o += n
    return out


def generated_answers(samples, tokens, n_new, eos_ids=()):
    """samples: the prompts' samples in batch order; tokens [n, max_new] / n_new [n] as returned by Context.generate (rows cut behind their first eos
    token). Returns per sample (gen, gen_correct): gen = the generated ids without the eos token, gen_correct = 1 when the first n_answer generated
    ids equal the reference answer ids."""
    eos = set(int(e) for e in eos_ids)
    out = []
    for i, smp in enumerate(samples):
        gen = [int(t) for t in np.asarray(tokens[i])[:int(n_new[i])]]
        if gen and gen[-1] in eos:
            gen = gen[:-1]
        ans = [int(t) for t in smp.ids[smp.n_prompt:]]
        out.append((gen, int(len(ans) > 0 and gen[:len(ans)] == ans)))
    return out


_M64 = (1 << 64) - 1


def sample_seeds(sample_seed, dataset_indices):
    """one uint64 per QA pair for Context.sample's seq_seeds: output number (index + 1) of the splitmix64 generator seeded with the run's sample_seed, i.e. the
    splitmix64 finaliser of sample_seed + (index + 1) * 0x9E3779B97F4A7C15 mod 2^64. It depends on the run's seed and the pair's index in the data set and on
    nothing else, so a pair's draws are the same function of its logits in every fold layout, batch order and stacking."""
    out = np.zeros(len(dataset_indices), np.uint64)
    for k, idx in enumerate(dataset_indices):
        z = (int(sample_seed) + (int(idx) + 1) * 0x9E3779B97F4A7C15) & _M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        out[k] = z ^ (z >> 31)
    return out


def sampled_answers(samples, tokens, logp, n_new, eos_ids=()):
    """samples: the prompts' samples in batch order; tokens / logp [n, n_samples, max_new] and n_new [n, n_samples] as returned by Context.sample (every draw cut
    behind its first eos token). Returns per sample dict(ids = the n_samples id lists without the eos token, logp = the summed log-probability of each draw (its
    eos token included: the probability of the whole answer at the sampling temperature), match = the share of draws whose first n_answer ids equal the reference
    answer ids)."""
    eos = set(int(e) for e in eos_ids)
    out = []
    for i, smp in enumerate(samples):
        ans = [int(t) for t in smp.ids[smp.n_prompt:]]
        ids, lps, hit = [], [], 0
        for k in range(np.asarray(tokens).shape[1]):
            m = int(n_new[i][k])
            gen = [int(t) for t in np.asarray(tokens[i][k])[:m]]
            lps.append(float(np.asarray(logp[i][k], np.float64)[:m].sum()))
            if gen and gen[-1] in eos:
                gen = gen[:-1]
            ids.append(gen)
            hit += int(len(ans) > 0 and gen[:len(ans)] == ans)
        out.append(dict(ids=ids, logp=lps, match=hit / max(len(ids), 1)))
    return out


CAND_MAX_LEN = 16   # TST_CAND_MAX_LEN (include/tst_hip.h): a longer answer is not a candidate


def answer_candidates(samples, top):
    """the `top` most frequent distinct reference answers (token-id tuples, ids[n_prompt:]) over the "na" samples of the whole data set, most frequent first; ties
    go to the answer that occurs first. Answers of more than CAND_MAX_LEN tokens (or none) are left out: tst_score_candidates_async does not take them."""
    count, first = {}, {}
    for i, x in enumerate(samples):
        if x.kind != "na":
            continue
        ans = tuple(int(t) for t in x.ids[x.n_prompt:])
        if not 1 <= len(ans) <= CAND_MAX_LEN:
            continue
        count[ans] = count.get(ans, 0) + 1
        first.setdefault(ans, i)
    return sorted(count, key=lambda a: (-count[a], first[a]))[:max(0, int(top))]


def sample_candidates(x, cands):
    """the candidates one held-out sample is scored on: none for an "mca" sample (its restricted softmax already is this); for an "na" sample the data set's list
    `cands` and, behind it, the sample's own reference answer when the list does not hold it (and it has 1 .. CAND_MAX_LEN tokens)"""
    if x.kind != "na":
        return []
    out = [tuple(c) for c in cands]
    ref = tuple(int(t) for t in x.ids[x.n_prompt:])
    if ref not in out and 1 <= len(ref) <= CAND_MAX_LEN:
        out.append(ref)
    return out


def pack_candidates(samples, cands):
    """(cand_ids, cu_cand, cand_seq) of a held-out batch for Context.score_candidates: sample_candidates of every sample, in batch order"""
    ids, cu, seq = [], [0], []
    for s, x in enumerate(samples):
        for c in sample_candidates(x, cands):
            ids += list(c)
            cu.append(len(ids))
            seq.append(s)
    return np.array(ids, np.int32), np.array(cu, np.int32), np.array(seq, np.int32)


def candidate_scores(samples, cands, logp_cand):
    """samples: a held-out batch in the order of pack_candidates(samples, cands); logp_cand: log p(candidate | prompt) of its candidates, flat, as
    Context.score_candidates_fetch returns them. Per sample None ("mca", or no candidate at all) or dict(n = candidates scored, cands = their id tuples,
    logp = their log-probabilities, p = softmax(logp) over the sample's list (float64), mass = logsumexp(logp): the share of the model's own distribution the list
    covers (as a log), rank = 1 + the number of candidates strictly more probable than the reference (None when the reference is not on the list), p_ref = the
    reference's p (None likewise), top / top_p = the five most probable candidates and their p, ties in list order)."""
    lp_all = np.asarray(logp_cand, np.float64).reshape(-1)
    n_all = sum(len(sample_candidates(x, cands)) for x in samples)
    if n_all != len(lp_all):
        raise ValueError(f"candidate_scores: {len(lp_all)} log-probabilities for {n_all} candidates")
    out, o = [], 0
    for x in samples:
        mine = sample_candidates(x, cands)
        if not mine:
            out.append(None)
            continue
        lp = lp_all[o:o + len(mine)]
        o += len(mine)
        m = float(lp.max())
        mass = m + float(np.log(np.exp(lp - m).sum()))
        p = np.exp(lp - mass)
        ref = tuple(int(t) for t in x.ids[x.n_prompt:])
        j = mine.index(ref) if ref in mine else None
        order = np.argsort(-lp, kind="stable")[:5]
        out.append(dict(n=len(mine), cands=mine, logp=lp.copy(), p=p, mass=mass, rank=None if j is None else 1 + int((lp > lp[j]).sum()),
                        p_ref=None if j is None else float(p[j]), top=[list(mine[k]) for k in order], top_p=[float(p[k]) for k in order]))
    return out
