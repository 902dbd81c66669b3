"""Python side of the prefix-tree Transformer-LM step (csrc/lm_tree.hip): the kernels' plan (what an LM must
look like), the tree state of a chunk of transducer searches (lists and lengths per state slot, node counters, status words, the K / V
node pools) and the step's parameter record.  engine.rnnt_beam_search_batch drives it under decoder.rnnt_tlm_fusion = "device", the
fused CTC search (modeling/ctc_beam_search.py, section 32) under decoder.ctc_tlm_fusion = "device": there the slots are the rows of
the LM pool and the rows of a step are the frame's records (advance_records, TreeStep(n))."""
import ctypes

import torch

from . import lib, ops

LDS_BYTES, ATTN_LDS_FIXED = 64 * 1024, 1536      # emoasr_lm_tree_attn: 8 Lcap bytes (scores + node list) + q, k, v of one head
OVERLEN, POOL_FULL = lib.LM_TREE_OVERLEN, lib.LM_TREE_POOL_FULL
STATUS = {OVERLEN: "a hypothesis outgrew the prefix capacity", POOL_FULL: "the node pool is full"}


def head_ok(d, H):
    """the attention kernel's plan for the heads: d / H in 8 .. 128, a multiple of 8 (as emoasr_attn_step)"""
    return H >= 1 and d % H == 0 and (d // H) % 8 == 0 and 8 <= d // H <= 128


def attn_lds_bytes(Lcap):
    return 8 * int(Lcap) + ATTN_LDS_FIXED


def list_cap(E, longest, max_seq_len):
    """Lcap: the longest prefix a slot may hold -- <sos> and E - 1 labels per frame, never more than the LM's positions"""
    return max(1, min(1 + (E - 1) * longest, int(max_seq_len)))


def node_cap(W, E, longest):
    """nodes per search, worst case: every fused round (E - 1 per frame) steps W rows, + 1 so that the capacity is never zero"""
    return W * (E - 1) * longest + 1


def ctc_list_cap(max_frames, max_seq_len):
    """Lcap of the fused CTC search: <eos> and at most one label per frame, never more than the LM's positions"""
    return max(1, min(1 + int(max_frames), int(max_seq_len)))


def ctc_node_cap(W, max_frames):
    """nodes per CTC search, worst case: the root and W new prefixes per frame (a prefix that drops out and forms again takes a
    fresh node)"""
    return int(W) * int(max_frames) + 1


def las_list_cap(max_len, max_seq_len):
    """Lcap of the fused LAS search (section 33): one token per step (<eos> first), never more than the LM's positions"""
    return max(1, min(int(max_len), int(max_seq_len)))


def las_node_cap(W, max_len):
    """nodes per LAS search, worst case: W live rows on every step, + 1 so that the capacity is never zero"""
    return int(W) * int(max_len) + 1


def las_search_bytes(W, Lcap, node_cap, layers, d, V, esz):
    """bytes of one LAS search's share of the tree: its node_cap nodes in both pools (K and V) of every layer, the lists and
    lengths of its 2 W slots, the step's logits (LM dtype) and the f32 rows the score kernel reads"""
    return 2 * layers * int(node_cap) * d * esz + 2 * int(W) * (int(Lcap) + 1) * 4 + int(W) * V * (esz + 4)


def _ptr(x):
    return ops._p(x) if torch.is_tensor(x) else x


class TreeState:
    """the tree of S searches of width W: llen / lanc per state slot, nnodes / status per search, (node, position) per row.  rows:
    the row capacity (S W when not given: the transducer's W rows per search; the CTC search's compact record list names its own)"""

    def __init__(self, S, W, nslots, Lcap, node_cap, device, rows=None):
        z = lambda *shape: torch.zeros(*shape, device=device, dtype=torch.int32)
        self.S, self.W, self.nslots, self.Lcap, self.node_cap = int(S), int(W), int(nslots), int(Lcap), int(node_cap)
        self.nodes = self.S * self.node_cap
        self.rows = self.S * self.W if rows is None else int(rows)
        assert self.rows >= self.S * self.W, "the whole-capacity entry points step S W rows"
        self.llen, self.lanc, self.nnodes, self.status = z(nslots), z(nslots, Lcap), z(S), z(S)
        self.row_node, self.row_pos = torch.full((self.rows,), -1, device=device, dtype=torch.int32), z(self.rows)
        self.ctl = None                                  # advance_records' control words (lab, dst): int64 [2, rows]
        c = self.c = lib.LmTree()
        c.S, c.W, c.nslots, c.Lcap, c.node_cap = self.S, self.W, self.nslots, self.Lcap, self.node_cap
        c.llen, c.lanc, c.nnodes = self.llen.data_ptr(), self.lanc.data_ptr(), self.nnodes.data_ptr()
        c.row_node, c.row_pos, c.status = self.row_node.data_ptr(), self.row_pos.data_ptr(), self.status.data_ptr()

    def reset(self):
        """before a search: every slot holds the empty prefix (a search's first slot is the zero state it starts from), no node is
        taken, no bit is raised"""
        self.llen.zero_()
        self.nnodes.zero_()
        self.status.zero_()

    def pools(self, layers, d, dtype):
        """-> (K, V) node pools [layers, nodes, d] of the compute dtype"""
        return tuple(torch.zeros(layers, self.nodes, d, device=self.llen.device, dtype=dtype) for _ in range(2))

    def advance(self, src, dst, active):
        """emoasr_lm_tree_advance under the control words src / dst / active (int64 [S W] tensors or device addresses)"""
        lib.call("emoasr_lm_tree_advance", ctypes.byref(self.c), _ptr(src), _ptr(dst), _ptr(active), ops._stream())

    def control_words(self):
        """-> int64 [2, rows] (lab, dst), the control words advance_records writes and the step reads; made on first use"""
        if self.ctl is None:
            self.ctl = torch.zeros(2, self.rows, device=self.llen.device, dtype=torch.int64)
            self.ctl[1].fill_(-1)
        return self.ctl

    def advance_records(self, rec, rec_count, lm_weight=None):
        """emoasr_lm_tree_advance_rec under the record list of the fused CTC search: rec int32 [6, rows], rec_count int32 [1] (it
        stays on the device); lm_weight f64 [S] or None: the records of a search with lm_weight <= 0 take no node"""
        assert tuple(rec.shape) == (6, self.rows) and ops._chk(rec, torch.int32).is_contiguous(), (tuple(rec.shape), self.rows)
        assert ops._chk(rec_count, torch.int32).numel() == 1
        assert lm_weight is None or (tuple(ops._chk(lm_weight, torch.float64).shape) == (self.S,) and lm_weight.is_contiguous())
        ctl = self.control_words()
        lib.call("emoasr_lm_tree_advance_rec", ctypes.byref(self.c), ops._p(rec), self.rows, ops._p(rec_count), ops._p(lm_weight),
                 ops._p(ctl[0]), ops._p(ctl[1]), ops._stream())

    def advance_beam(self, ids, parent, state, src_base, dst_base):
        """emoasr_lm_tree_advance_beam under the lockstep book of the batched LAS search (section 33): ids / parent int32 [S W],
        state int32 [S, 4]; row r reads slot src_base + its parent's row and writes slot dst_base + r.  The control words are
        the tree's own (control_words)."""
        nb = self.S * self.W
        for x in (ids, parent):
            assert ops._chk(x, torch.int32).numel() == nb and x.is_contiguous(), (tuple(x.shape), nb)
        assert tuple(ops._chk(state, torch.int32).shape) == (self.S, 4) and state.is_contiguous()
        ctl = self.control_words()
        lib.call("emoasr_lm_tree_advance_beam", ctypes.byref(self.c), ops._p(ids), ops._p(parent), ops._p(state), int(src_base),
                 int(dst_base), ops._p(ctl[0]), ops._p(ctl[1]), ops._stream())

    def attn(self, qkv, kpool, vpool, dst, H, out=None, n=None):
        """emoasr_lm_tree_attn on ONE layer's pools [nodes, d]: qkv [S W, 3 d] -> out [S W, d] (rows without a node are not written);
        n: emoasr_lm_tree_attn_rows over the first n of `rows` rows"""
        R, d = (self.S * self.W if n is None else self.rows), qkv.shape[1] // 3
        assert tuple(qkv.shape) == (R, 3 * d) and ops._chk(qkv).is_contiguous()
        for pool in (kpool, vpool):
            assert tuple(pool.shape) == (self.nodes, d) and ops._chk(pool, qkv.dtype).is_contiguous()
        if out is None:
            out = torch.zeros(R, d, device=qkv.device, dtype=qkv.dtype)
        assert tuple(out.shape) == (R, d) and ops._chk(out, qkv.dtype).is_contiguous()
        if n is None:
            lib.call("emoasr_lm_tree_attn", ops.dt(qkv), ctypes.byref(self.c), d, int(H), ops._p(qkv), ops._p(kpool), ops._p(vpool),
                     _ptr(dst), ops._p(out), ops._stream())
        else:
            assert 0 <= int(n) <= R, (n, R)
            lib.call("emoasr_lm_tree_attn_rows", ops.dt(qkv), ctypes.byref(self.c), int(n), d, int(H), ops._p(qkv), ops._p(kpool),
                     ops._p(vpool), _ptr(dst), ops._p(out), ops._stream())
        return out

    def raise_for_status(self, who, names=None, tags=False):
        """a raised bit is reported, not swallowed: RuntimeError naming the searches and the limit they met (tags: and the bit's name,
        OVERLEN / POOL_FULL)"""
        bits = self.status.tolist()
        if not any(bits):
            return
        parts = []
        for s, b in enumerate(bits):
            if b:
                name = names[s] if names is not None else f"search {s}"
                why = []
                if b & OVERLEN:
                    why.append(f"{STATUS[OVERLEN]} of {self.Lcap} tokens" + (" [OVERLEN]" if tags else ""))
                if b & POOL_FULL:
                    why.append(f"{STATUS[POOL_FULL]} ({self.node_cap} nodes per search)" + (" [POOL_FULL]" if tags else ""))
                parts.append(f"{name}: " + " and ".join(why))
        raise RuntimeError(f"{who}: " + "; ".join(parts))


class TreeStep:
    """emoasr_lm_tree_step of a Transformer LM (modeling/lm.py, lm_type "transformer") on a TreeState: raw logits [rows, V] of the
    compute dtype for the rows of the control words lab / dst (not given: the tree's own, which advance_records writes).  step() is
    the whole capacity, step(n) emoasr_lm_tree_step_rows over the first n rows.  The parameter addresses are read when it is built
    (after lm._prepare()): build it anew when the arena moved."""

    def __init__(self, lm, tree, lab=None, dst=None):
        if lab is None:
            lab, dst = tree.control_words()
        from .decode_rt import LMStepRuntime, _lin, _ln
        P = lm.params
        A, self.layers = LMStepRuntime(lm)._params()
        d, H, F, V, nl = P.hidden_size, P.num_attention_heads, P.intermediate_size, P.vocab_size, P.num_layers
        dev, dtype = A.flat.device, A.shadow.dtype
        assert lm._pe.shape[0] >= tree.Lcap and lm._pe.dtype == torch.float32, (tuple(lm._pe.shape), tree.Lcap)
        self.tree, self.nl, self.R, self.V = tree, nl, tree.rows, V
        self.kpool, self.vpool = tree.pools(nl, d, dtype)
        self.logits = torch.zeros(self.R, V, device=dev, dtype=dtype)
        code = lib.BF16 if dtype == torch.bfloat16 else lib.F32
        self.ws = torch.zeros(lib.size_query("emoasr_lm_tree_step_ws_bytes", code, self.R, d, F), device=dev, dtype=torch.uint8)
        pre, cp = "lm.transformer.bert.", "lm.transformer.cls.predictions."
        io = self.io = lib.LmTreeStep()
        io.d, io.H, io.F, io.V, io.n_emb = d, H, F, V, V
        io.lab, io.dst = _ptr(lab), _ptr(dst)
        io.word_emb, io.pe = A.w(pre + "embeddings.word_embeddings.weight").data_ptr(), lm._pe.data_ptr()
        _ln(io.ln_emb, A.p(pre + "embeddings.LayerNorm.weight"), A.p(pre + "embeddings.LayerNorm.bias"))
        io.kpool, io.vpool = self.kpool.data_ptr(), self.vpool.data_ptr()
        _lin(io.transform, A.w(cp + "transform.dense.weight"), A.p(cp + "transform.dense.bias"))
        _ln(io.ln_transform, A.p(cp + "transform.LayerNorm.weight"), A.p(cp + "transform.LayerNorm.bias"))
        io.out_bias, io.logits = A.p(cp + "bias").data_ptr(), self.logits.data_ptr()
        io.ws, io.ws_bytes = self.ws.data_ptr(), self.ws.numel()

    def __call__(self, n=None):
        if n is None:
            lib.call("emoasr_lm_tree_step", ops.dt(self.logits), self.nl, self.layers, ctypes.byref(self.tree.c), ctypes.byref(self.io),
                     ops._stream())
        else:
            assert 0 <= int(n) <= self.R, (n, self.R)
            lib.call("emoasr_lm_tree_step_rows", ops.dt(self.logits), self.nl, self.layers, ctypes.byref(self.tree.c),
                     ctypes.byref(self.io), int(n), ops._stream())
        return self.logits
