"""Reference for the batched transducer greedy search in lockstep (csrc/rnnt_greedy_batch.hip).  TEST INFRASTRUCTURE ONLY.

    Lockstep(Ts, K, blank, eos, max_seq_len)   the bookkeeping of oracle.rnnt.rnnt_greedy for S searches that move together: every
                                               step scores up to K consecutive frames of a live search against its current state,
                                               the first non-blank row is the next emission; two state slots per search, swapped on
                                               every LSTM step; the cut after the label that makes len(hyp) > max_seq_len
        .ctl(offs)                             the control words the NEXT step runs under, in the kernel's layout and numbering
        .advance(argmax_of)                    one step from argmax_of(search, window row) -> id
    search(scorer, Ts, K, ...)                 the whole search over scorer(search, label sequence, frame) -> arg-max id
                                               -> (hyps, aligns, steps): steps[n] = the words and the live count before step n,
                                               the last entry after the end
    hash_rows(seed, V, blank, ...)             synthetic logit rows: a hash of (seed, search, label sequence, frame) seeds the row

A label sequence is the hypothesis with the leading <sos> (= eos)."""
import zlib

import numpy as np

BLANK, EOS = 0, 2


class Lockstep:
    def __init__(self, Ts, K, blank=BLANK, eos=EOS, max_seq_len=256):
        assert 1 <= K <= 16
        self.Ts, self.K, self.blank, self.eos, self.max_seq_len = [int(T) for T in Ts], K, blank, eos, max_seq_len
        self.S = len(self.Ts)
        self.t = [0] * self.S
        self.cur = [1] * self.S                       # the slot (0 / 1 of the search's pair) that holds its current state
        self.done = [T == 0 for T in self.Ts]         # a search without frames: finished from the start, [] and []
        self.hyps = [[] for _ in self.Ts]
        self.aligns = [[] for _ in self.Ts]
        # the LSTM row of the next step, local slots: (label, src, dst, active); <eos> from the zeroed slot 0 into slot 1
        self.lstm = [(0, 0, 0, 0) if d else (eos, 0, 1, 1) for d in self.done]

    @property
    def live(self):
        return sum(1 for d in self.done if not d)

    def joint(self, s):
        """the K joint rows of search s in the next step, local numbering: (slot, active, frame)"""
        rows = []
        for i in range(self.K):
            on = not self.done[s] and self.t[s] + i < self.Ts[s]
            rows.append((self.cur[s], 1, self.t[s] + i) if on else (0, 0, 0))
        return rows

    def ctl(self, offs):
        """int64 [4 S + 3 S K]: [4][S] label, source slot, destination slot, active; [3][S K] slot, active, row of the stacked
        frames (offs[s] frames lie before search s).  Search s owns the slots 2 s and 2 s + 1; inactive rows are zero."""
        S, K = self.S, self.K
        w = np.zeros(4 * S + 3 * S * K, dtype=np.int64)
        lw, jw = w[:4 * S].reshape(4, S), w[4 * S:].reshape(3, S * K)
        for s in range(S):
            lab, src, dst, on = self.lstm[s]
            if on:
                lw[:, s] = (lab, 2 * s + src, 2 * s + dst, 1)
            for i, (slot, on, t) in enumerate(self.joint(s)):
                if on:
                    jw[:, s * K + i] = (2 * s + slot, 1, int(offs[s]) + t)
        return w

    def advance(self, argmax_of):
        for s in range(self.S):
            if self.done[s]:
                continue
            n = min(self.K, self.Ts[s] - self.t[s])
            assert n >= 1
            self.lstm[s] = (0, 0, 0, 0)
            k, tok = 0, self.blank
            while k < n:
                tok = int(argmax_of(s, k))
                if tok != self.blank:
                    break
                k += 1
            self.aligns[s] += [self.blank] * k
            self.t[s] += k
            if k < n:    # the label is emitted AT frame t + k: the search stays on it
                self.aligns[s].append(tok)
                self.hyps[s].append(tok)
                if len(self.hyps[s]) > self.max_seq_len:      # (the reference breaks AFTER the label that exceeds the limit)
                    self.done[s] = True
                else:
                    self.lstm[s] = (tok, self.cur[s], 1 - self.cur[s], 1)
                    self.cur[s] = 1 - self.cur[s]
            elif self.t[s] == self.Ts[s]:
                self.done[s] = True


def search(scorer, Ts, K, blank=BLANK, eos=EOS, max_seq_len=256):
    L = Lockstep(Ts, K, blank, eos, max_seq_len)
    offs = np.concatenate([[0], np.cumsum(L.Ts)])
    steps = []
    bound = max(L.Ts, default=0) + max_seq_len + 1
    while True:
        steps.append(dict(lstm=list(L.lstm), joint=[L.joint(s) for s in range(L.S)], ctl=L.ctl(offs), live=L.live))
        if L.live == 0:
            break
        assert len(steps) <= bound, (len(steps), bound)
        L.advance(lambda s, i: scorer(s, tuple([eos] + L.hyps[s]), L.t[s] + i))
    return L.hyps, L.aligns, steps


def hash_rows(seed, V, blank=BLANK, p_blank=0.5, tie=False, never_blank=False):
    """rows(search, label sequence, frame) -> float32 [V].  With probability p_blank the blank entry is lifted to the row's
    maximum + 1 (tie: to the maximum itself, so that the lower index of blank and the other maximum wins).  tie: values on the
    integers -3 .. 3 -- exact in bfloat16, many exact ties.  never_blank: the blank entry below every other."""
    def rows(s, seq, t):
        h = zlib.crc32(np.asarray([seed, s, t, len(seq)] + list(seq), dtype=np.int64).tobytes())
        rng = np.random.default_rng(h)
        x = rng.normal(size=V) * 2.0
        if tie:
            x = np.clip(np.round(x), -3, 3)
        lift = rng.random() < p_blank
        if never_blank:
            x[blank] = x.min() - 1.0
        elif lift:
            x[blank] = x.max() + (0.0 if tie else 1.0)
        return x.astype(np.float32)
    return rows


def argmax_scorer(rows):
    """the first maximum of a row, as emoasr_argmax_rows takes it"""
    return lambda s, seq, t: int(np.argmax(rows(s, seq, t)))
