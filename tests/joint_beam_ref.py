"""numpy restatement of ONE batched beam update (csrc/decode_batch.hip: emoasr_beam_update_batch) over S searches of width W:
float32 candidate scores with numpy's rounding, float64 hypothesis scores, the two stable rank orders, <eos> -> result with
+ len_weight * (pos + 2), empty hypotheses dropped, a search stops at W results or without a live beam, unused slots are
copies of the search's slot 0, n_parent is a global row, the shared position advances once per live step.

    st = new_state(S, W, max_pos, eos)
    update(st, vals, cands, psi, lm_at, cw, eos, lam, mu, len_weight)     # in place, one step
    hyps, scores = results(st)
"""
import numpy as np


def new_state(S, W, max_pos, eos):
    nb = S * W
    return dict(S=S, W=W, max_pos=max_pos, pos=0, all_done=0, mirror=[0, 0],
                state=np.tile(np.array([0, 1, 0, 0], dtype=np.int32), (S, 1)),     # pos, n_alive, n_results, done
                ids=np.full(nb, eos, np.int32), last=np.full(nb, eos, np.int32),
                parent=(np.arange(nb, dtype=np.int32) // W) * W, pcand=np.zeros(nb, np.int32),
                outlen=np.zeros(nb, np.int32), klens=np.ones(nb, np.int32),
                score=np.zeros(nb, np.float64), score_ctc=np.zeros(nb, np.float32),
                hist_parent=np.zeros((max_pos, nb), np.int32), hist_token=np.zeros((max_pos, nb), np.int32),
                res_score=np.zeros(nb, np.float64), res_step=np.zeros(nb, np.int32), res_parent=np.zeros(nb, np.int32))


def update(st, vals, cands, psi, lm_at, cw, eos, lam, mu, len_weight):
    """vals f32 / cands i32 [nb, cw]; psi, lm_at f32 [nb, cw] or None; lam = decode_ctc_weight, mu = lm_weight"""
    S, W = st["S"], st["W"]
    if st["all_done"] or st["pos"] >= st["max_pos"]:
        return
    pos = st["pos"]
    f1, fl, fm = np.float32(1 - lam), np.float32(lam), np.float32(mu)
    for s in range(S):
        state = st["state"][s]
        if state[3]:
            continue
        R, na = s * W, int(state[1])
        cand = []     # (hypothesis score f64, m, j) in (m, rank) order
        keep = min(W, cw)
        for m in range(na):
            if psi is not None:
                sc = f1 * vals[R + m] + fl * (psi[R + m] - st["score_ctc"][R + m])
                if lm_at is not None:
                    sc = sc + fm * lm_at[R + m]
            else:
                sc = vals[R + m].copy()
            assert sc.dtype == np.float32
            for j in np.argsort(-sc, kind="stable")[:keep]:
                cand.append((float(st["score"][R + m]) + float(sc[j]), m, int(j)))
        order = sorted(range(len(cand)), key=lambda e: -cand[e][0])[:W]    # (sorted is stable)
        a, nres = 0, int(state[2])
        n_ids, n_parent, n_pcand = np.zeros(W, np.int32), np.zeros(W, np.int32), np.zeros(W, np.int32)
        n_score, n_ctc = np.zeros(W, np.float64), np.zeros(W, np.float32)
        hp, ht = np.full(W, -1, np.int32), np.full(W, -1, np.int32)
        for e in order:
            c, m, j = cand[e]
            tok = int(cands[R + m, j])
            if tok == eos:
                if pos < 1:
                    continue
                st["res_score"][R + nres] = c + len_weight * float(pos + 2)
                st["res_step"][R + nres] = pos
                st["res_parent"][R + nres] = m
                nres += 1
                if nres >= W:
                    break
            else:
                n_ids[a], n_parent[a], n_pcand[a] = tok, R + m, j
                n_score[a] = c
                n_ctc[a] = psi[R + m, j] if psi is not None else 0.0
                hp[a], ht[a] = m, tok
                a += 1
        for k in range(a, W):
            n_ids[k] = n_ids[0] if a > 0 else eos
            n_parent[k] = n_parent[0] if a > 0 else R
            n_pcand[k] = n_pcand[0] if a > 0 else 0
        rows = slice(R, R + W)
        st["ids"][rows], st["parent"][rows], st["pcand"][rows] = n_ids, n_parent, n_pcand
        st["score"][rows], st["score_ctc"][rows] = n_score, n_ctc
        st["hist_parent"][pos, rows], st["hist_token"][pos, rows] = hp, ht
        st["last"][rows] = n_ids
        st["outlen"][rows] = pos + 1
        st["klens"][rows] = pos + 2
        state[1], state[2] = a, nres
        state[3] = 1 if (nres >= W or a == 0) else 0
        state[0] = pos + 1
    # the tail: once per live step
    nd = int(st["state"][:, 3].sum())
    st["pos"] = pos + 1
    if nd == S:
        st["all_done"] = 1
    st["mirror"] = [pos + 1, nd]


def results(st):
    """-> (hyps[s], scores[s]): the token lists rebuilt from the history, each search's results sorted by score (stable)"""
    S, W = st["S"], st["W"]
    hyps, scores = [], []
    for s in range(S):
        R, out = s * W, []
        for k in range(int(st["state"][s, 2])):
            toks, slot = [], int(st["res_parent"][R + k])
            for p in range(int(st["res_step"][R + k]) - 1, -1, -1):
                toks.append(int(st["hist_token"][p, R + slot]))
                slot = int(st["hist_parent"][p, R + slot])
            out.append((toks[::-1], float(st["res_score"][R + k])))
        out = sorted(out, key=lambda r: r[1], reverse=True)
        hyps.append([r[0] for r in out])
        scores.append([r[1] for r in out])
    return hyps, scores
