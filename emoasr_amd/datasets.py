"""On-disk data formats of the reference, host side: the TSV manifest + per-utterance `.npy` feature
files (asr/datasets.py:25-177), the length-budgeted batch sampler (:180-245), the decode result TSV
(asr/test_asr.py:265-313) and the vocabulary file (utils/vocab.py).

    manifest columns   feat_path  utt_id  token_id  text  xlen  ylen     (tab separated, header row)
    feat_path          float array [frames, >= feat_dim] saved with np.save; the first feat_dim columns are used
    token_id           space-separated integer ids (no <eos>)

Differences from the reference are deliberate and local: SpecAugment is NOT applied per utterance on
the CPU here -- the batch's mask spans are sampled with the reference's draws (data.specaug_spans) and
applied by one HIP kernel on the padded batch (ops.specaug_apply).

Optional inputs of the auxiliary branches, same formats as the reference: phone targets (manifest columns
phone_token_id / phone_text, datasets.py:43-64,108-116 -> batch keys ps / plens / ptexts, padded with
params.phone_eos_id) and knowledge-distillation soft labels (params.kd_label_path: a pickle
{utt_id without speed-perturbation prefix: [per label position: [(token id, probability), ...]]},
datasets.py:70-79,118-131,248-263 -> batch key soft_labels [B, L(+1), V]).
"""
import logging
import random

import numpy as np
import torch

from .data import pack_batches


def _read_table(path):
    import pandas as pd
    return pd.read_table(path, comment="#")


def get_utt_id_nosp(utt_id):
    """utils/converters.py:17-26: drop the speed-perturbation prefix "sp0.9-" / "sp1.0-" / "sp1.1-" """
    if utt_id.startswith(("sp0.9", "sp1.0", "sp1.1")):
        return "-".join(utt_id.split("-")[1:])
    return utt_id


def create_soft_label(data_kd_utt, ylen, vocab_size, lsm_prob, add_eos=False, eos_id=2):
    """datasets.py:248-263: per label position the teacher's top-k probabilities scaled by 1-lsm_prob, the
    smoothing mass spread over the other classes; positions the teacher does not cover stay all-zero;
    with add_eos one more row for <eos> (attention decoders: same length as ys_out)."""
    soft = torch.zeros(ylen + 1 if add_eos else ylen, vocab_size)
    for i, topk in enumerate(data_kd_utt):
        soft[i, :] = lsm_prob / (vocab_size - len(topk))
        for v, prob in topk:
            soft[i, v] = float(np.float64(prob)) * (1 - lsm_prob)
    if add_eos:
        soft[-1, :] = lsm_prob / (vocab_size - 1)
        soft[-1, eos_id] = 1.0 * (1 - lsm_prob)
    return soft


class ASRDataset:
    """Items: (utt_id, x float32 [T, feat_dim * num_framestacks], xlen, y int64 [L], ylen, text,
    p int64 [P] | None, plen | None, ptext | None, soft_label f32 [L(+1), V] | None)."""

    COLUMNS = ["feat_path", "utt_id", "token_id", "text", "xlen", "ylen"]

    def __init__(self, params, data_path, phase="train", size=-1, decode_phone=False):
        self.feat_dim = params.feat_dim
        self.num_framestacks = getattr(params, "num_framestacks", 1)
        self.vocab_size = getattr(params, "vocab_size", None)
        self.lsm_prob = getattr(params, "lsm_prob", 0.0)
        self.eos_id = params.eos_id
        self.phase = phase
        columns = list(self.COLUMNS)
        self.with_phones = (phase == "train" and getattr(params, "mtl_phone_ctc_weight", 0) > 0) or decode_phone
        if self.with_phones:
            columns += ["phone_token_id", "phone_text"]
            self.phone_eos_id = params.phone_eos_id
        self.data = _read_table(data_path)[columns]
        self.data_kd = None
        if phase == "train" and (getattr(params, "kd_weight", 0) > 0 or getattr(params, "inter_kd_weight", 0) > 0):
            import pickle
            with open(params.kd_label_path, "rb") as f:
                self.data_kd = pickle.load(f)
            logging.info(f"kd labels: {params.kd_label_path}")
            self.add_eos = params.decoder_type in ["transformer", "las"]
        if size > 0:
            self.data = self.data[:size]
        self.data = self.data.reset_index(drop=True)

    def __len__(self):
        return len(self.data)

    def __getitem__(self, idx):
        row = self.data.loc[idx]
        x = torch.from_numpy(np.load(row["feat_path"])[:, : self.feat_dim].astype(np.float32))
        if self.num_framestacks > 1:  # datasets.py:134-142: drop the ragged tail, concatenate consecutive frames
            n = x.shape[0] // self.num_framestacks
            x = x[: n * self.num_framestacks].reshape(n, self.feat_dim * self.num_framestacks)
        y = torch.tensor([int(t) for t in str(row["token_id"]).split()], dtype=torch.long)
        p = plen = ptext = soft = None
        if self.with_phones:
            p = torch.tensor([int(t) for t in str(row["phone_token_id"]).split()], dtype=torch.long)
            plen, ptext = p.shape[0], row["phone_text"]
        if self.data_kd is not None:
            key = get_utt_id_nosp(row["utt_id"])
            if key not in self.data_kd:
                logging.warning(f"soft label: {key} not found")
            soft = create_soft_label(self.data_kd.get(key, []), y.shape[0], self.vocab_size, self.lsm_prob,
                                     add_eos=self.add_eos, eos_id=self.eos_id)
        return row["utt_id"], x, x.shape[0], y, y.shape[0], row["text"], p, plen, ptext, soft

    def collate_fn(self, batch):
        """dict with the reference's keys (datasets.py:144-177): xs zero-padded, ys padded with <eos>
        (no <eos> appended), ys_in = <eos> + y, ys_out = y + <eos> (both <eos>-padded, length ylen+1)."""
        utt_ids, xs, xlens, ys, ylens, texts, ps, plens, ptexts, softs = zip(*batch)
        eos = self.eos_id
        B, T, L = len(xs), max(xlens), max(ylens)
        xpad = torch.zeros(B, T, xs[0].shape[1])
        ypad = torch.full((B, L), eos, dtype=torch.long)
        yin = torch.full((B, L + 1), eos, dtype=torch.long)
        yout = torch.full((B, L + 1), eos, dtype=torch.long)
        for b in range(B):
            xpad[b, : xlens[b]] = xs[b]
            ypad[b, : ylens[b]] = ys[b]
            yin[b, 1: ylens[b] + 1] = ys[b]
            yout[b, : ylens[b]] = ys[b]
        ret = {"utt_ids": list(utt_ids), "texts": list(texts), "xs": xpad, "xlens": torch.tensor(xlens),
               "ys": ypad, "ylens": torch.tensor(ylens, dtype=torch.long), "ys_in": yin, "ys_out": yout}
        if ps[0] is not None:
            ppad = torch.full((B, max(plens)), self.phone_eos_id, dtype=torch.long)
            for b in range(B):
                ppad[b, : plens[b]] = ps[b]
            ret.update(ps=ppad, plens=torch.tensor(plens), ptexts=list(ptexts))
        if softs[0] is not None:
            spad = torch.zeros(B, max(s.shape[0] for s in softs), softs[0].shape[1])
            for b in range(B):
                spad[b, : softs[b].shape[0]] = softs[b]
            ret["soft_labels"] = spad
        return ret


class ASRBatchSampler:
    """Consecutive utterances of the (length-sorted) manifest are packed until the next one would exceed
    max_xlens_batch input frames, max_ylens_batch labels or batch_size utterances; batches with fewer
    than min_batch_size utterances are dropped (datasets.py:200-234).  The batch ORDER is reshuffled at
    every epoch (:236-242), the composition of each batch never changes."""

    def __init__(self, dataset, params, min_batch_size=1, seed=0):
        xlens, ylens = dataset.data["xlen"].values, dataset.data["ylen"].values
        assert xlens.max(initial=0) <= params.max_xlens_batch and ylens.max(initial=0) <= params.max_ylens_batch, \
            "an utterance exceeds the per-batch budget"
        self.indices_batches = pack_batches(xlens, ylens, params.max_xlens_batch, params.max_ylens_batch,
                                            params.batch_size, min_batch_size)
        dropped = len(xlens) - sum(len(b) for b in self.indices_batches)
        if dropped:
            logging.warning(f"{dropped} utterances are skipped because their batch is smaller than min_batch_size")
        self._rng = random.Random(seed)

    def __iter__(self):
        self._rng.shuffle(self.indices_batches)
        return iter(self.indices_batches)

    def __len__(self):
        return len(self.indices_batches)

    def shard(self, rank, world):
        """this rank's batches for one-process-per-GPU data parallelism: batch i goes to rank i % world
        (every rank sees the same shuffled order; the tail is dropped so all ranks step equally often)"""
        n = len(self.indices_batches) // world * world
        return [self.indices_batches[i] for i in range(rank, n, world)]


def batches(dataset, sampler):
    for idx in sampler:
        yield dataset.collate_fn([dataset[i] for i in idx])


class Vocab:
    """`token id` per line (utils/vocab.py:5-43); sentencepiece-style subwords -> words (:45-64)."""

    def __init__(self, vocab_path):
        self.i2t, self.t2i = {}, {}
        with open(vocab_path) as f:
            for line in f:
                if not line.strip():
                    continue
                token, idx = line.split()
                self.i2t[int(idx)] = token
                self.t2i[token] = int(idx)
        self.unk_id = self.t2i["<unk>"]

    def id2token(self, idx):
        return self.i2t[idx]

    def ids2tokens(self, ids):
        return [self.i2t[i] for i in ids]

    def token2id(self, token):
        return self.t2i.get(token, self.unk_id)

    def tokens2ids(self, tokens):
        return [self.token2id(t) for t in tokens]

    def ids2words(self, ids):
        return self.subwords_to_words(self.ids2tokens(ids))

    def ids2text(self, ids):
        return " ".join(self.ids2words(ids))

    @staticmethod
    def subwords_to_words(subwords):
        """a new word starts at a piece beginning with the sentencepiece marker or with `<`, and right
        after a piece ending in `>` (special tokens stand alone)"""
        words, cur = [], ""
        for piece in subwords:
            if piece[0] in ("▁", "<") or (cur and cur[-1] == ">"):
                if cur:
                    words.append(cur)
                cur = piece[1:] if piece[0] == "▁" else piece
            else:
                cur += piece
        if cur:
            words.append(cur)
        return words


def write_results_tsv(path, rows, comment=None):
    """decode results in the reference's layout (test_asr.py:265-313): utt_id, token_id, text, reftext
    (+ any extra keys of the row dicts), tab separated; an optional `# ...` comment line (WER summary)
    goes first, as utils/log.py:insert_comment does."""
    keys = ["utt_id", "token_id", "text", "reftext"]
    extra = [k for k in rows[0] if k not in keys] if rows else []
    with open(path, "w") as f:
        if comment:
            f.write("# " + comment + "\n")
        f.write("\t".join(keys + extra) + "\n")
        for r in rows:
            tok = r["token_id"]
            tok = tok if isinstance(tok, str) else " ".join(str(int(t)) for t in tok)
            f.write("\t".join([str(r["utt_id"]), tok, str(r["text"]), str(r["reftext"])] + [str(r[k]) for k in extra]) + "\n")


def create_masked_lm_label(y, mask_id, num_to_mask=-1, mask_proportion=-1, random_num_to_mask=False, eos_id=2):
    """lm/datasets.py:319-341: mask `num_to_mask` (or max(int(candidates * mask_proportion), 1); with random_num_to_mask a uniform
    draw from 1..that) of the positions whose token is not <eos>, always with mask_id -> (y_masked, labels int64, -100 where not
    masked).  The `random` calls come in the reference's order (shuffle, randint, sample): the same seed gives the same masks."""
    y_masked = y.clone()
    label = torch.full(y.shape, -100, dtype=torch.int64)
    cands = [j for j in range(y.size(0)) if y[j] != eos_id]
    random.shuffle(cands)
    if mask_proportion > 0:
        num_to_mask = max(int(len(cands) * mask_proportion), 1)
    if random_num_to_mask:
        num_to_mask = random.randint(1, num_to_mask)
    for j in sorted(random.sample(cands, num_to_mask)):
        label[j] = y[j]
        y_masked[j] = mask_id
    return y_masked, label


class LMDataset:
    """lm/datasets.py:24-120 for the Transformer, the RNN, the BERT masked LM and ELECTRA: a TSV with columns utt_id / token_id
    (space-separated ids).  Items: (utt_id, y_in int64, ylen, label int64 | None), for "electra-disc" with a fifth entry error_label float64.  With params.add_sos_eos the ids are wrapped in
    <eos>.  phase "train": y_in = y[:-1] and label = y[1:] (next-token targets) for lm_type "transformer" / "rnn"; for "bert"
    y_in = y with mask_id at the masked positions and label = the hidden tokens there, -100 elsewhere (create_masked_lm_label;
    exactly one of params.num_to_mask / params.mask_proportion is configured); "electra" masks as "bert" does, with the same `random`
    call order.  "electra-disc" reads a third column error_label -- space-separated tags, one per token; a token's target is 1 when
    its tag is not "C" -- keeps y_in = y without labels, and its batches carry `error_labels` padded with -100.  Any other phase:
    y_in = y, no label."""

    def __init__(self, params, data_path, phase="train", size=-1):
        if params.lm_type not in ("transformer", "rnn", "bert", "electra", "electra-disc"):     # (next-token targets for the first two: lm/datasets.py:91)
            raise NotImplementedError(f"emoasr_amd: LMDataset for lm_type={params.lm_type!r} is outside the HIP hot path")
        if params.lm_type == "electra-disc":
            columns = ["utt_id", "token_id", "error_label"]
        else:
            columns = ["utt_id", "token_id"] + (["ylen"] if getattr(params, "bucket_shuffle", False) else [])
        data = _read_table(data_path)[columns]
        n = len(data)
        data = data.dropna().reset_index(drop=True)
        if len(data) != n:
            logging.warning(f"nan value in dataset is removed: {n:d} -> {len(data):d}")
        self.lm_type = params.lm_type
        self.add_sos_eos = params.add_sos_eos
        self.eos_id = params.eos_id
        self.phase = phase
        self.data = data[:size] if size > 0 else data
        self.masked = self.lm_type in ("bert", "electra")
        if self.masked:
            # a config written for another LM family (no mask token, no masking rule) is not one this dataset can be built from
            missing = [f for f in ("mask_id", "random_num_to_mask") if not hasattr(params, f)]
            if missing:
                raise NotImplementedError(f"emoasr_amd: lm_type={self.lm_type!r} needs the masked LM's fields; {missing} are absent from the config")
            self.mask_id = params.mask_id
            # either `num_to_mask` or `mask_proportion` must be specified (lm/datasets.py:56)
            assert hasattr(params, "num_to_mask") ^ hasattr(params, "mask_proportion")
            self.num_to_mask = getattr(params, "num_to_mask", -1)
            self.mask_proportion = getattr(params, "mask_proportion", -1)
            self.random_num_to_mask = params.random_num_to_mask

    def __len__(self):
        return len(self.data)

    def __getitem__(self, idx):
        row = self.data.loc[idx]
        ids = [int(t) for t in str(row["token_id"]).split()]
        if self.add_sos_eos:
            ids = [self.eos_id] + ids + [self.eos_id]
        y = torch.tensor(ids, dtype=torch.long)
        err = None
        if "error_label" in self.data:     # (lm/datasets.py:76-78)
            err = torch.tensor([e != "C" for e in str(row["error_label"]).split()], dtype=torch.float64)
        if self.phase == "train" and self.masked:
            y_in, label = create_masked_lm_label(y, self.mask_id, self.num_to_mask, self.mask_proportion, self.random_num_to_mask,
                                                 self.eos_id)
        elif self.phase == "train" and self.lm_type in ("transformer", "rnn"):
            assert len(y) > 1
            y_in, label = y[:-1], y[1:]
        else:
            y_in, label = y, None
        item = (row["utt_id"], y_in, y_in.size(0), label)
        return item if err is None else item + (err,)

    def collate_fn(self, batch):
        """dict with the reference's keys: ys_in padded with <eos>, ylens, labels padded with -100 (train phase only), error_labels
        padded with -100 ("electra-disc")"""
        from torch.nn.utils.rnn import pad_sequence
        utt_ids, ys_in, ylens, labels = list(zip(*batch))[:4]
        errs = [it[4] for it in batch] if len(batch[0]) > 4 else None
        ret = {"utt_ids": list(utt_ids), "ys_in": pad_sequence(ys_in, batch_first=True, padding_value=self.eos_id),
               "ylens": torch.tensor(ylens)}
        if labels[0] is not None:
            ret["labels"] = pad_sequence(labels, batch_first=True, padding_value=-100)
        if errs is not None:
            ret["error_labels"] = pad_sequence(errs, batch_first=True, padding_value=-100)
        return ret


# ---- phone-to-word data (lm/datasets.py:123-369, lm/text_augment.py) --------------------------------------------------------------
def create_masked_lm_label_insert(y, mask_id, num_to_mask=-1, mask_proportion=-1, random_num_to_mask=False, insert_poisson_lam=-1,
                                  pad_id=0, eos_id=2):
    """lm/datasets.py:344-369: create_masked_lm_label, then a Poisson(insert_poisson_lam) number of extra <mask> tokens after every
    position (numpy's global generator, one draw of len(y) values after the `random` calls of the masking); an inserted mask's
    label is pad_id.  -> (y_masked_insert, labels int64)"""
    y_masked, label = create_masked_lm_label(y, mask_id, num_to_mask, mask_proportion, random_num_to_mask, eos_id)
    if not insert_poisson_lam > 0:     # (the reference returns unbound names here; its dataset never calls it so)
        return y_masked, label
    num_inserts = np.random.poisson(insert_poisson_lam, len(y_masked))
    n = len(y_masked) + int(sum(num_inserts))
    y_ins = torch.full([n], mask_id, dtype=torch.int64)
    label_ins = torch.full([n], pad_id, dtype=torch.int64)
    index = 0
    for tok, lab, k in zip(y_masked, label, num_inserts):
        y_ins[index], label_ins[index] = tok, lab
        index += 1 + int(k)
    return y_ins, label_ins


class TextAugment:
    """lm/text_augment.py:12-55 on a phone sequence: up to int(len * textaug_max_mask_prob) positions become phone_mask_id, then up
    to int(len * textaug_max_replace_prob) positions get a random phone; <eos> positions are never touched.  The `random` calls
    come in the reference's order (randint, sample; randint, sample, choices)."""

    def __init__(self, params):
        self.max_mask_prob = params.textaug_max_mask_prob
        self.max_replace_prob = params.textaug_max_replace_prob
        self.phone_vocab_size = params.src_vocab_size
        self.eos_id = params.phone_eos_id
        self.mask_id = params.phone_mask_id

    def __call__(self, x):
        return self._text_replace(self._text_mask(x))

    def _text_mask(self, x):
        x_masked = x.clone()
        if self.max_mask_prob <= 0:
            return x_masked
        num_to_mask = random.randint(0, int(len(x) * self.max_mask_prob))
        cands = [j for j in range(len(x)) if x[j] != self.eos_id]
        x_masked[random.sample(cands, min(len(cands), num_to_mask))] = self.mask_id
        return x_masked

    def _text_replace(self, x):
        x_replaced = x.clone()
        if self.max_replace_prob <= 0:
            return x_replaced
        num_to_replace = random.randint(0, int(len(x) * self.max_replace_prob))
        cands = [j for j in range(len(x)) if x[j] != self.eos_id]
        indices = random.sample(cands, min(len(cands), num_to_replace))
        vocab = [j for j in range(self.phone_vocab_size) if j != self.eos_id]
        # (more replacements asked for than candidates: the shapes differ and the assignment fails, as in the reference)
        x_replaced[indices] = torch.tensor(random.choices(vocab, k=num_to_replace), dtype=torch.long)
        return x_replaced


class P2WDataset:
    """lm/datasets.py:123-243: a TSV with columns utt_id / token_id / phone_token_id (and ylen / plen with params.bucket_shuffle).
    Items: (utt_id, p int64, plen, y_in int64, ylen, label | None).  phase "train": the phones go through TextAugment when
    params.text_augment; "pbert" masks the words (create_masked_lm_label, or create_masked_lm_label_insert with
    params.mask_insert_poisson_lam > 0), and so does "pelectra" (modeling/pelectra.py: lm/datasets.py:159,195); "pctc" has y_in = y and
    label = p, as the reference does.  Any other phase: no label."""

    def __init__(self, params, data_path, phase="train", size=-1):
        if params.lm_type not in ("pbert", "pctc", "pelectra"):
            raise NotImplementedError(f"emoasr_amd: P2WDataset for lm_type={params.lm_type!r} is outside the HIP hot path")
        columns = ["utt_id", "token_id", "phone_token_id"] + (["ylen", "plen"] if getattr(params, "bucket_shuffle", False) else [])
        data = _read_table(data_path)[columns]
        n = len(data)
        data = data.dropna().reset_index(drop=True)
        if len(data) != n:
            logging.warning(f"nan value in dataset is removed: {n:d} -> {len(data):d}")
        self.lm_type = params.lm_type
        self.add_sos_eos = params.add_sos_eos
        self.eos_id, self.phone_eos_id = params.eos_id, params.phone_eos_id
        self.phase = phase
        self.data = data[:size] if size > 0 else data
        self.textaug = TextAugment(params) if phase == "train" and params.text_augment else None
        self.masked = self.lm_type in ("pbert", "pelectra")
        if self.masked:
            self.mask_id = params.mask_id
            assert hasattr(params, "num_to_mask") ^ hasattr(params, "mask_proportion")     # (lm/datasets.py:162)
            self.num_to_mask = getattr(params, "num_to_mask", -1)
            self.mask_proportion = getattr(params, "mask_proportion", -1)
            self.random_num_to_mask = params.random_num_to_mask
            self.mask_insert_poisson_lam = getattr(params, "mask_insert_poisson_lam", -1)
            self.pad_id = getattr(params, "pad_id", 0)

    def __len__(self):
        return len(self.data)

    def __getitem__(self, idx):
        row = self.data.loc[idx]
        ids = [int(t) for t in str(row["token_id"]).split()]
        if self.add_sos_eos:
            ids = [self.eos_id] + ids + [self.eos_id]
        y = torch.tensor(ids, dtype=torch.long)
        p = torch.tensor([int(t) for t in str(row["phone_token_id"]).split()], dtype=torch.long)
        if self.textaug is not None:
            p = self.textaug(p)
        if self.phase == "train" and self.masked:
            if self.mask_insert_poisson_lam > 0:
                y_in, label = create_masked_lm_label_insert(y, self.mask_id, self.num_to_mask, self.mask_proportion,
                                                            self.random_num_to_mask, self.mask_insert_poisson_lam, self.pad_id,
                                                            self.eos_id)
            else:
                y_in, label = create_masked_lm_label(y, self.mask_id, self.num_to_mask, self.mask_proportion,
                                                     self.random_num_to_mask, self.eos_id)
        elif self.phase == "train":
            y_in, label = y, p
        else:
            y_in, label = y, None
        return row["utt_id"], p, p.size(0), y_in, y_in.size(0), label

    def collate_fn(self, batch):
        """dict with the reference's keys: ps padded with the phone <eos>, plens, ys_in padded with <eos>, ylens, labels (-100)"""
        from torch.nn.utils.rnn import pad_sequence
        utt_ids, ps, plens, ys_in, ylens, labels = zip(*batch)
        ret = {"utt_ids": list(utt_ids), "ps": pad_sequence(ps, batch_first=True, padding_value=self.phone_eos_id),
               "plens": torch.tensor(plens), "ys_in": pad_sequence(ys_in, batch_first=True, padding_value=self.eos_id),
               "ylens": torch.tensor(ylens)}
        if labels[0] is not None:
            ret["labels"] = pad_sequence(labels, batch_first=True, padding_value=-100)
        return ret


class LMBatchSampler:
    """lm/datasets.py:247-316: consecutive utterances until sum(plen) > max_plens_batch (P2W data; absent: no phone limit),
    sum(ylen) > max_ylens_batch or batch_size utterances; the batches are shuffled each epoch with the `random` module"""

    def __init__(self, dataset, params, min_batch_size=1):
        ylens = dataset.data["ylen"].values
        plens = dataset.data["plen"].values if "plen" in dataset.data else np.zeros(len(ylens), dtype=np.int64)
        max_plens = getattr(params, "max_plens_batch", 1)     # (without phones every plen counts 0)
        assert plens.max(initial=0) <= max_plens and ylens.max(initial=0) <= params.max_ylens_batch
        self.indices_batches, i, n = [], 0, len(ylens)
        while i < n:
            cur, sp, sy = [], 0, 0
            while i < n and not (sp + plens[i] > max_plens or sy + ylens[i] > params.max_ylens_batch
                                 or len(cur) + 1 > params.batch_size):
                cur.append(i)
                sp, sy, i = sp + plens[i], sy + ylens[i], i + 1
            if len(cur) < min_batch_size:
                logging.warning(f"{len(cur)} utterances are skipped because of they are smaller than min_batch_size")
            else:
                self.indices_batches.append(cur)

    def __iter__(self):
        random.shuffle(self.indices_batches)
        yield from self.indices_batches

    def __len__(self):
        return len(self.indices_batches)
