"""KGE models on PyTorch-ROCm tensors whose scoring runs in libkge_hip.so.

Two drop-in classes share the tables and the fused HIP scoring path:

* ``TFKGEModel`` mirrors ``tensorflow_codes/model.py:47-235`` — constructor flags (including the
  dead ``-dr`` flag, Q5), ``model_func`` plugin dict, and ``call(((pos, neg), mode))`` returning
  ``[B, 1]``: ``logsigmoid(score)`` for mode 3 (model.py:145) and the self-adversarial reduction
  ``sum softmax(s) * logsigmoid(-s)`` for the negative modes (model.py:168-171,195-198; Q1, Q3, Q4).
* ``KGEModel`` mirrors the upstream PyTorch ``KnowledgeGraphEmbedding/codes/model.py``
  (absent from the snapshot; restated from its published code): ``forward(sample, mode)`` returns
  raw scores ``[B, 1|N]`` and the static ``train_step`` / ``test_step`` drive training / eval.

Deliberate deviation from the TF graph: ``call`` evaluates only the branch the mode
selects instead of all three blended with 0/1 masks. Outputs are identical except that the
reference would turn a NaN/Inf in an unused branch into a NaN output (0 * NaN); we do not.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from ._lib import FN_IDS, HEAD_BATCH, SINGLE, TAIL_BATCH

SPLIT_ENTITY = {"ComplEx", "RotatE", "InterHT"}


def _dims_for(model_name, entity_dim, relation_dim):
    """Per-half width D and relation offset for a score function, validating the table widths the
    way the reference's broadcasting would (it raises on a mismatch)."""
    if model_name in ("TransE", "DistMult", "pRotatE"):
        if entity_dim != relation_dim:
            raise ValueError(f"{model_name} needs entity_dim == relation_dim, got {entity_dim} / {relation_dim}")
        return entity_dim, 0
    if model_name == "ComplEx":
        if entity_dim % 2 or relation_dim != entity_dim:
            raise ValueError("ComplEx needs double entity and double relation embeddings")
        return entity_dim // 2, 0
    if model_name == "RotatE":
        if entity_dim % 2 or relation_dim * 2 != entity_dim:
            raise ValueError("RotatE needs a double entity embedding and a single relation embedding")
        return entity_dim // 2, 0
    if model_name == "InterHT":
        # model.py:208-210: entity split in 2, relation split in 3, middle third used (Q6)
        if entity_dim % 2 or relation_dim % 3 or entity_dim // 2 != relation_dim // 3:
            raise ValueError("InterHT needs -de and -tr (entity 2d, relation 3d)")
        return entity_dim // 2, entity_dim // 2
    if model_name == "PairRE":
        # upstream PairRE: the relation row holds (r_h | r_t), each as wide as the unsplit entity row
        if relation_dim != 2 * entity_dim:
            raise ValueError(f"PairRE needs relation_dim == 2 * entity_dim (-dr, no -de), got {entity_dim} / "
                             f"{relation_dim}")
        return entity_dim, 0
    if model_name == "TranSparse":
        # model.py:227: head [.., d] @ (mask * W)[d, d] and the relation row of width d
        if entity_dim != relation_dim:
            raise ValueError("TranSparse needs entity_dim == relation_dim")
        return entity_dim, 0
    raise ValueError(f"model {model_name} not supported")


def check_adam_moments(param, state):
    """The fused train steps address m / v with the PARAMETER's leading dimension (kge_hip.h: m_ent and
    v_ent use ent_ld, m_rel and v_rel use rel_ld), so a moment laid out differently from its parameter
    (a dense moment of a row-padded table, a state restored with other strides) would be read and
    written out of place, past its end for a padded table. Refuse it before any pointer is passed."""
    for key in ("exp_avg", "exp_avg_sq"):
        mom = state[key]
        same = tuple(mom.shape) == tuple(param.shape) and all(
            n <= 1 or a == b for n, a, b in zip(param.shape, mom.stride(), param.stride()))
        if not same:
            raise ValueError(
                f"Adam moment {key} has shape {tuple(mom.shape)} / strides {tuple(mom.stride())} but its "
                f"parameter has {tuple(param.shape)} / {tuple(param.stride())}: the fused step addresses "
                "both with the parameter's leading dimension")
        if mom.dtype != torch.float32 or mom.device != param.device:
            raise ValueError(f"Adam moment {key} must be float32 on {param.device}")


class _KGEBase(nn.Module):
    """Tables + the fused scoring entry shared by both model classes."""

    def _init_tables(self, nentity, nrelation, entity_dim, relation_dim, init_range, device, seed):
        g = torch.Generator().manual_seed(int(seed))
        ent = torch.empty(nentity, entity_dim).uniform_(-init_range, init_range, generator=g)
        rel = torch.empty(nrelation, relation_dim).uniform_(-init_range, init_range, generator=g)
        self.entity_embedding = nn.Parameter(ent.to(device))
        self.relation_embedding = nn.Parameter(rel.to(device))
        return g

    def _make_model_func(self):
        def plugin(name):
            fn = FN_IDS.get(name)

            def model_func(head, relation, tail, mode, *extra):
                m = ops.mode_id(mode)
                if name == "TranSparse":
                    return self._transparse_dense(head, relation, m, *extra)
                ew = head.shape[-1]
                D = ew // 2 if name in SPLIT_ENTITY else ew
                rel_off = D if name == "InterHT" else 0
                mod = float(self.modulus.detach().reshape(-1)[0]) if name == "pRotatE" else 0.0
                return ops.score_dense(fn, m, head, relation, tail, D, self._gamma_f, self._range_f,
                                       rel_off=rel_off, modulus=mod)

            model_func.__name__ = name
            return model_func

        return {name: plugin(name) for name in list(FN_IDS) + ["TranSparse"]}

    def _transparse_dense(self, head, relation, mode, weight, mask):
        """model_func['TranSparse'](head, relation, tail, mode, weight, mask) on pre-gathered rows
        (model.py:226-235): the gathered tensors become the kernel's tables, indexed 0..rows-1."""
        B, d = head.shape[0], head.shape[-1]
        dev = head.device
        ar = torch.arange(B, device=dev, dtype=torch.int64)
        pos = torch.stack([ar, ar, ar], dim=1)
        rel = relation.reshape(B, d)
        if mode == HEAD_BATCH:
            N = head.shape[1]
            ent = head.reshape(B * N, d)
            neg = torch.arange(B * N, device=dev, dtype=torch.int64).view(B, N)
        else:
            ent = head.reshape(B, d)
            neg = None
        return ops.transparse_score(mode, ent.contiguous(), rel.contiguous(), weight.contiguous(),
                                    mask.contiguous().to(torch.float32), pos, neg, self._gamma_f)

    # fused gather + score (no [B, N, d] tensor is ever built)
    @property
    def supports_fused_step(self):
        return self.model_name in FN_IDS

    def score(self, mode, positive_sample, negative_sample=None):
        if self.model_name == "TranSparse":
            return ops.transparse_score(mode, self.entity_embedding, self.relation_embedding, self.W, self.mask,
                                        positive_sample, negative_sample, self._gamma_f)
        fn = FN_IDS[self.model_name]
        modulus = self.modulus if self.model_name == "pRotatE" else None
        return ops.score_indexed(fn, mode, self.entity_embedding, self.relation_embedding,
                                 positive_sample, negative_sample, self._D, self._gamma_f,
                                 self._range_f, rel_off=self._rel_off, modulus=modulus)

    def predict(self, queries, mode, k=10, known_triples=None, batch_size=None, filter_on="device"):
        """The k best entities (ids [M, k] int64, scores [M, k]) for each query (h, r, ?) (tail-batch) or (?, r, t)
        (head-batch), without the answers `known_triples` (triples, or an evaluate.FilterTable of them) already
        hold: evaluate.predict."""
        from . import evaluate

        return evaluate.predict(self, queries, mode, k=k, known_triples=known_triples, batch_size=batch_size,
                                filter_on=filter_on)

    def extra_repr(self):
        return (f"model_name={self.model_name}, nentity={self.nentity}, nrelation={self.nrelation}, "
                f"entity_dim={self.entity_dim}, relation_dim={self.relation_dim}, gamma={self._gamma_f}")

    # shared by the fused train steps of both classes (kge_train_step, kge_train_step_reg)
    def _train_workspace(self, nbytes, device):
        """kge_train_step's workspace, cached by size (the call zeroes the counters it keeps there
        itself, so the contents never matter: any shape may reuse a large-enough buffer)."""
        ws = getattr(self, "_train_ws", None)
        if ws is None or ws.numel() < nbytes or ws.device != device:
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
            self._train_ws = ws
        return ws

    def _adam_state(self, optimizer, params):
        """(group, lr, step) for the next update. The step counters are NOT advanced here: the caller
        commits them with _adam_commit only after the kernel call returned success, so a rejected
        call leaves the bias correction where it was."""
        from .optim import resolve_lr

        group = optimizer.param_groups[0]
        st0 = optimizer.state[self.entity_embedding]
        lr = resolve_lr(group["lr"], st0["step"] if st0 else 0)
        for prm in params:
            st = optimizer.state[prm]
            if not st:
                st["step"] = 0
                st["exp_avg"] = ops.like_strided(prm, zero=True)
                st["exp_avg_sq"] = ops.like_strided(prm, zero=True)
            check_adam_moments(prm, st)
        return group, lr, optimizer.state[self.entity_embedding]["step"] + 1

    @staticmethod
    def _adam_commit(optimizer, params):
        for prm in params:
            optimizer.state[prm]["step"] += 1


class TFKGEModel(_KGEBase):
    """Drop-in for ``TFKGEModel`` (tensorflow_codes/model.py:47-235)."""

    def __init__(self, model_name, nentity, nrelation, hidden_dim, gamma,
                 double_entity_embedding=False, double_relation_embedding=False,
                 triple_relation_embedding=False, device=None, seed=0, **kwargs):
        super().__init__()
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.model_name = model_name
        self.nentity = nentity
        self.nrelation = nrelation
        self.hidden_dim = hidden_dim
        self.epsilon = 2.0  # model.py:58
        g32 = torch.tensor([gamma], dtype=torch.float32)
        self.gamma = nn.Parameter(g32.clone(), requires_grad=False)  # model.py:60
        # model.py:62-63: (gamma.numpy() + epsilon) / hidden_dim, evaluated in float32
        rng = (g32 + torch.tensor(self.epsilon, dtype=torch.float32)) / hidden_dim
        self.embedding_range = nn.Parameter(rng.clone(), requires_grad=False)

        # model.py:65-78 — Q5: the -dr result is overwritten by the -tr branch, so -dr is dead.
        # ComplEx and PairRE cannot be built at all without a double relation, so there (only) -dr is honoured.
        relation_dim = hidden_dim * 2 if double_relation_embedding else hidden_dim
        entity_dim = hidden_dim * 2 if double_entity_embedding else hidden_dim
        if triple_relation_embedding:
            relation_dim = hidden_dim * 3
        elif not (model_name in ("ComplEx", "PairRE") and double_relation_embedding):
            relation_dim = hidden_dim
        self.entity_dim, self.relation_dim = entity_dim, relation_dim

        # model.py:86-91 (Q8): U(-(gamma+2)/d, (gamma+2)/d) for both tables (torch RNG, seeded)
        g = self._init_tables(nentity, nrelation, entity_dim, relation_dim, float(rng[0]), device, seed)
        if model_name == "TranSparse":
            # model.py:96-106: per relation a fixed 0/1 mask (uniform[1, 100) >= int(0.5 * 100)) and a
            # trainable W [R, rd, rd] drawn with the same initializer (torch RNG, seeded)
            prob = torch.empty(nrelation, relation_dim, relation_dim).uniform_(1.0, 100.0, generator=g)
            self.register_buffer("mask", (prob >= 50).to(torch.float32).to(device))
            W = torch.empty(nrelation, relation_dim, relation_dim).uniform_(-float(rng[0]), float(rng[0]), generator=g)
            self.W = nn.Parameter(W.to(device))
        if model_name == "InterHT":
            self.u = 1  # model.py:94-95 (the kernel hard-codes u = 1)
        if model_name == "pRotatE":
            self.modulus = nn.Parameter(torch.tensor([[0.5 * float(rng[0])]], device=device))
        self._gamma_f = float(g32[0])
        self._range_f = float(rng[0])
        self._D, self._rel_off = _dims_for(model_name, entity_dim, relation_dim)
        self.model_func = self._make_model_func()  # model.py:109-112

    def forward(self, sample, training=True, **kwargs):
        """``call(((positive_sample, negative_sample), mode))`` -> [B, 1] (model.py:114-205)."""
        (positive_sample, negative_sample), mode = sample
        m = ops.mode_id(mode)
        if m == SINGLE:  # positive_call -> single_mode (model.py:117-146)
            return ops.log_sigmoid(self.score(SINGLE, positive_sample))
        # negative_call (model.py:121-125): head_batch_mode if mode == 0 else tail_batch_mode
        s = self.score(m, positive_sample, negative_sample)
        return ops.neg_reduce(s, temperature=1.0, adversarial=True, detach=False).unsqueeze(1)

    call = forward

    def step_forward(self, positive_sample, negative_sample, mode):
        """Both calls of supervisor.py:17-18 fused into one launch (kge_step_forward):
        returns (self(((pos, neg), mode)), self(((pos, neg), 3))), each [B, 1], differentiable."""
        m = ops.mode_id(mode)
        if m == SINGLE:
            raise ValueError("step_forward needs the batch's negative mode")
        if self.model_name == "TranSparse":
            params = (self.entity_embedding, self.relation_embedding, self.W)
            if torch.is_grad_enabled() and any(t.requires_grad for t in params):
                return self(((positive_sample, negative_sample), m)), self(((positive_sample, negative_sample), SINGLE))
            # no autograd: both calls and their reductions in one entry point (bitwise the two calls above)
            M = ops.transparse_premul(self.W, self.mask) if ops._want_premul(self.W, positive_sample,
                                                                              negative_sample, m) else None
            _, on, _, op = ops.transparse_step_forward_raw(m, self.entity_embedding, self.relation_embedding, self.W,
                                                           self.mask, positive_sample, negative_sample, self._gamma_f,
                                                           M=M)
            return on.unsqueeze(1), op.unsqueeze(1)
        modulus = self.modulus if self.model_name == "pRotatE" else None
        neg, pos = ops.step_forward(FN_IDS[self.model_name], m, self.entity_embedding,
                                    self.relation_embedding, positive_sample, negative_sample,
                                    self._D, self._gamma_f, self._range_f, rel_off=self._rel_off,
                                    modulus=modulus, temperature=1.0, adversarial=True, detach=False)
        return neg.unsqueeze(1), pos.unsqueeze(1)

    def train_step_fused(self, positive_sample, negative_sample, subsampling_weight, mode, optimizer,
                         one_call=True, loss_sum=None):
        """supervisor.py:15-26 entirely in HIP. Needs `optimizer` =
        customknowledgegraphembedding_amd.optim.Adam over this model's parameters; returns the loss
        (0-dim tensor).
          one_call (default): kge_train_step — forward with phase 1 of the backward fused in (each
            candidate row gathered once per step), one epilogue launch (loss, score gradients, query
            chains, event buckets), deterministic backward with Adam fused into the entity pass.
          one_call=False (and pRotatE): kge_step_forward, kge_step_loss, kge_step_backward_adam —
            bitwise equal to the autograd path (kge_step_backward + kge_adam_update).
          loss_sum: optional 0-dim fp32 device tensor the loss is added to (one_call only; a running
            Sum metric updated inside the step's last kernel).
        Raises ValueError when an Adam moment is not laid out like its parameter (check_adam_moments)."""
        from .optim import Adam
        from . import _lib

        if not isinstance(optimizer, Adam):
            raise TypeError("train_step_fused needs customknowledgegraphembedding_amd.optim.Adam")
        if not self.supports_fused_step:
            raise NotImplementedError(f"{self.model_name} has no fused train step; use the autograd path")
        lazy = _lazy_group(optimizer)
        if lazy and self.model_name == "pRotatE":
            raise NotImplementedError("pRotatE has no lazy train step (kge_train_step_lazy)")
        if lazy and not one_call:
            raise ValueError("a lazy Adam needs the one-call train step (one_call=True)")
        m = ops.mode_id(mode)
        fn = FN_IDS[self.model_name]
        ent, rel = self.entity_embedding, self.relation_embedding
        is_p = self.model_name == "pRotatE"
        # moments the optimizer already holds (restored, or made elsewhere) are checked before anything is
        # launched; the ones this step creates are laid out like their parameter (_adam_state)
        for prm in [ent, rel] + ([self.modulus] if is_p else []):
            if optimizer.state[prm]:
                check_adam_moments(prm, optimizer.state[prm])
        if one_call and not is_p:
            return self._train_step_one_call(fn, m, positive_sample, negative_sample, subsampling_weight, optimizer,
                                             loss_sum, lazy)
        if loss_sum is not None:
            loss = self.train_step_fused(positive_sample, negative_sample, subsampling_weight, mode, optimizer,
                                         one_call=False)
            loss_sum += loss
            return loss
        modulus = float(self.modulus.detach().reshape(-1)[0]) if is_p else 0.0
        stats = (torch.empty((negative_sample.shape[0] * negative_sample.shape[1], 2), dtype=torch.float32,
                             device=ent.device) if self.model_name == "InterHT" else None)
        out_neg, out_pos, ns, ps = ops.step_forward_raw(fn, m, ent.detach(), rel.detach(), self._rel_off,
                                                        positive_sample, negative_sample, self._D, self._gamma_f,
                                                        self._range_f, modulus, cand_stats=stats)
        # supervisor.py:19-23 and its gradient in one launch (the same kernel as the autograd path)
        loss, d_out = ops.step_loss_raw(out_neg, out_pos, subsampling_weight)
        group, lr, step = self._adam_state(optimizer, [ent, rel] + ([self.modulus] if is_p else []))
        b1, b2 = group["betas"]
        B, N = ns.shape
        lib = _lib.load()
        nbytes = lib.kge_step_backward_adam_workspace_size(fn, ent.shape[0], rel.shape[0], rel.stride(0), B, N,
                                                           self._D)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=ent.device)
        sm = optimizer.state[self.modulus] if is_p else None
        rc = lib.kge_step_backward_adam(
            fn, m, ent.data_ptr(), ent.shape[0], ent.stride(0), rel.data_ptr(), rel.shape[0], rel.stride(0),
            self._rel_off, positive_sample.data_ptr(), negative_sample.data_ptr(), negative_sample.stride(0), B, N,
            self._D, self._gamma_f, self._range_f, self.modulus.data_ptr() if is_p else None, modulus, 1.0, 1, 0,
            ns.data_ptr(), ns.stride(0), ps.data_ptr(), d_out.data_ptr(), d_out.data_ptr(),
            optimizer.state[ent]["exp_avg"].data_ptr(), optimizer.state[ent]["exp_avg_sq"].data_ptr(),
            optimizer.state[rel]["exp_avg"].data_ptr(), optimizer.state[rel]["exp_avg_sq"].data_ptr(),
            sm["exp_avg"].data_ptr() if is_p else None, sm["exp_avg_sq"].data_ptr() if is_p else None,
            float(lr), float(b1), float(b2), float(group["eps"]), int(step), int(group["semantics"] == "keras"),
            None if stats is None else stats.data_ptr(), ws.data_ptr(), ws.numel(),
            torch.cuda.current_stream(ent.device).cuda_stream)
        _lib.check(rc, "kge_step_backward_adam")
        self._adam_commit(optimizer, [ent, rel] + ([self.modulus] if is_p else []))
        return loss.detach()

    def _train_step_one_call(self, fn, m, positive_sample, negative_sample, subsampling_weight, optimizer,
                             loss_sum=None, lazy=False):
        """kge_train_step (a lazy Adam group: kge_train_step_lazy): supervisor.py:15-26 in one C-ABI call."""
        from . import _lib

        ent, rel = self.entity_embedding, self.relation_embedding
        ops._need_gpu(ent, positive_sample, negative_sample, subsampling_weight)
        if loss_sum is not None and (loss_sum.dtype != torch.float32 or loss_sum.device != ent.device):
            raise ValueError("loss_sum must be a float32 tensor on the model's device")
        dev = ent.device
        pos = positive_sample.contiguous()
        neg = negative_sample
        if neg.stride(1) != 1:
            neg = neg.contiguous()
        w = subsampling_weight.reshape(-1).to(torch.float32).contiguous()
        B, N = neg.shape
        group, lr, step = self._adam_state(optimizer, [ent, rel])
        b1, b2 = group["betas"]
        lib = _lib.load()
        size_fn, step_fn, name = lib.kge_train_step_workspace_size, lib.kge_train_step, "kge_train_step"
        if lazy:
            size_fn, step_fn, name = lib.kge_train_step_lazy_workspace_size, lib.kge_train_step_lazy, name + "_lazy"
        nbytes = size_fn(fn, ent.shape[0], rel.shape[0], rel.stride(0), B, N, self._D)
        ws = self._train_workspace(nbytes, dev)
        out = torch.empty(2 * B + 1, dtype=torch.float32, device=dev)  # loss | out_neg | out_pos
        rc = step_fn(
            fn, m, ent.data_ptr(), ent.shape[0], ent.stride(0), rel.data_ptr(), rel.shape[0], rel.stride(0),
            self._rel_off, pos.data_ptr(), neg.data_ptr(), neg.stride(0), B, N, self._D, self._gamma_f,
            self._range_f, 1.0, 1, 0, w.data_ptr(), out.data_ptr(),
            None if loss_sum is None else loss_sum.data_ptr(), out[1:].data_ptr(), out[1 + B:].data_ptr(),
            optimizer.state[ent]["exp_avg"].data_ptr(), optimizer.state[ent]["exp_avg_sq"].data_ptr(),
            optimizer.state[rel]["exp_avg"].data_ptr(), optimizer.state[rel]["exp_avg_sq"].data_ptr(),
            float(lr), float(b1), float(b2), float(group["eps"]), int(step), int(group["semantics"] == "keras"),
            ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream, *((None,) if lazy else ()))
        _lib.check(rc, name)
        self._adam_commit(optimizer, [ent, rel])
        return out[0]


class KGEModel(_KGEBase):
    """Drop-in for the upstream PyTorch ``KGEModel`` (KnowledgeGraphEmbedding/codes/model.py)."""

    def __init__(self, model_name, nentity, nrelation, hidden_dim, gamma,
                 double_entity_embedding=False, double_relation_embedding=False,
                 device=None, seed=0):
        super().__init__()
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.model_name = model_name
        self.nentity = nentity
        self.nrelation = nrelation
        self.hidden_dim = hidden_dim
        self.epsilon = 2.0
        self.gamma = nn.Parameter(torch.Tensor([gamma]), requires_grad=False)
        self.embedding_range = nn.Parameter(
            torch.Tensor([(self.gamma.item() + self.epsilon) / hidden_dim]), requires_grad=False)
        self.entity_dim = hidden_dim * 2 if double_entity_embedding else hidden_dim
        self.relation_dim = hidden_dim * 2 if double_relation_embedding else hidden_dim
        if model_name not in ("TransE", "DistMult", "ComplEx", "RotatE", "pRotatE", "InterHT", "PairRE"):
            raise ValueError("model %s not supported" % model_name)
        if model_name == "PairRE" and (double_entity_embedding or not double_relation_embedding):
            raise ValueError("PairRE should use --double_relation_embedding")
        if model_name == "RotatE" and (not double_entity_embedding or double_relation_embedding):
            raise ValueError("RotatE should use --double_entity_embedding")
        if model_name == "ComplEx" and (not double_entity_embedding or not double_relation_embedding):
            raise ValueError("ComplEx should use --double_entity_embedding and --double_relation_embedding")
        rng = self.embedding_range.item()
        self._init_tables(nentity, nrelation, self.entity_dim, self.relation_dim, rng, device, seed)
        if model_name == "pRotatE":
            self.modulus = nn.Parameter(torch.Tensor([[0.5 * rng]]).to(device))
        self._gamma_f = float(self.gamma.item())
        self._range_f = float(self.embedding_range.item())
        self._D, self._rel_off = _dims_for(model_name, self.entity_dim, self.relation_dim)
        self.model_func = self._make_model_func()

    def forward(self, sample, mode="single"):
        if mode == "single":
            return self.score(SINGLE, sample)
        if mode == "head-batch":
            tail_part, head_part = sample
            return self.score(HEAD_BATCH, tail_part, head_part)
        if mode == "tail-batch":
            head_part, tail_part = sample
            return self.score(TAIL_BATCH, head_part, tail_part)
        raise ValueError("mode %s not supported" % mode)

    @staticmethod
    def train_step(model, optimizer, train_iterator, args):
        """Upstream ``KGEModel.train_step``: one optimisation step on one batch; returns the log."""
        model.train()
        optimizer.zero_grad()
        positive_sample, negative_sample, subsampling_weight, mode = next(train_iterator)
        dev = model.entity_embedding.device
        positive_sample = positive_sample.to(dev, non_blocking=True)
        negative_sample = negative_sample.to(dev, non_blocking=True)
        subsampling_weight = subsampling_weight.to(dev, non_blocking=True).reshape(-1)

        # both scoring calls and their reductions in one kge_step_forward launch; the backward is the
        # deterministic two-phase pass (detach: upstream detaches the self-adversarial weights)
        adv = bool(args.negative_adversarial_sampling)
        temp = float(args.adversarial_temperature) if adv else 1.0
        modulus = model.modulus if model.model_name == "pRotatE" else None
        negative_score, positive_score = ops.step_forward(
            FN_IDS[model.model_name], ops.mode_id(mode), model.entity_embedding, model.relation_embedding,
            positive_sample, negative_sample, model._D, model._gamma_f, model._range_f, rel_off=model._rel_off,
            modulus=modulus, temperature=temp, adversarial=adv, detach=True)

        if args.uni_weight:
            positive_sample_loss = -positive_score.mean()
            negative_sample_loss = -negative_score.mean()
        else:
            positive_sample_loss = -(subsampling_weight * positive_score).sum() / subsampling_weight.sum()
            negative_sample_loss = -(subsampling_weight * negative_score).sum() / subsampling_weight.sum()
        loss = (positive_sample_loss + negative_sample_loss) / 2
        if args.regularization != 0.0:
            regularization = args.regularization * (
                model.entity_embedding.norm(p=3) ** 3 + model.relation_embedding.norm(p=3).norm(p=3) ** 3)
            loss = loss + regularization
            regularization_log = {"regularization": regularization.item()}
        else:
            regularization_log = {}
        loss.backward()
        optimizer.step()
        log = {
            **regularization_log,
            "positive_sample_loss": positive_sample_loss.item(),
            "negative_sample_loss": negative_sample_loss.item(),
            "loss": loss.item(),
        }
        return log

    @staticmethod
    def train_step_fused(model, optimizer, train_iterator, args):
        """``train_step``'s signature and log in one kge_train_step_reg call: forward, upstream's loss with its
        flags (``uni_weight``, ``negative_adversarial_sampling`` / ``adversarial_temperature`` with detached
        weights, the L3 ``regularization``), deterministic backward and Adam, no dense gradient table.
        ``optimizer`` must be this package's ``optim.Adam`` (either ``semantics``) over the model's parameters,
        else TypeError; an Adam moment laid out unlike its parameter is a ValueError (check_adam_moments) before
        anything is launched. pRotatE has no such step: NotImplementedError, use ``train_step``. The log's four
        values come back in one device-to-host copy."""
        from .optim import Adam
        from . import _lib

        if not isinstance(optimizer, Adam):
            raise TypeError("train_step_fused needs customknowledgegraphembedding_amd.optim.Adam")
        if model.model_name == "pRotatE":
            raise NotImplementedError("pRotatE has no fused train step (kge_train_step_reg); use KGEModel.train_step")
        lazy = _lazy_group(optimizer)
        if lazy and float(args.regularization) != 0.0:
            raise ValueError("a lazy Adam cannot take the L3 regulariser: its gradient is dense "
                             "(regularization must be 0)")
        model.train()
        positive_sample, negative_sample, subsampling_weight, mode = next(train_iterator)
        ent, rel = model.entity_embedding, model.relation_embedding
        dev = ent.device
        pos = positive_sample.to(dev, non_blocking=True).contiguous()
        neg = negative_sample.to(dev, non_blocking=True)
        if neg.stride(1) != 1:
            neg = neg.contiguous()
        w = None
        if not args.uni_weight:
            w = subsampling_weight.to(dev, non_blocking=True).reshape(-1).to(torch.float32).contiguous()
        ops._need_gpu(ent, pos, neg)
        for prm in (ent, rel):
            if optimizer.state[prm]:
                check_adam_moments(prm, optimizer.state[prm])
        adv = bool(args.negative_adversarial_sampling)
        temp = float(args.adversarial_temperature) if adv else 1.0
        reg = float(args.regularization)
        fn, m = FN_IDS[model.model_name], ops.mode_id(mode)
        B, N = neg.shape
        group, lr, step = model._adam_state(optimizer, [ent, rel])
        b1, b2 = group["betas"]
        lib = _lib.load()
        size_fn, step_fn, name = lib.kge_train_step_reg_workspace_size, lib.kge_train_step_reg, "kge_train_step_reg"
        if lazy:
            size_fn, step_fn = lib.kge_train_step_lazy_workspace_size, lib.kge_train_step_lazy
            name = "kge_train_step_lazy"
        nbytes = size_fn(fn, ent.shape[0], rel.shape[0], rel.stride(0), B, N, model._D)
        ws = model._train_workspace(nbytes, dev)
        out = torch.empty(2 * B + 5, dtype=torch.float32, device=dev)  # log[4] | loss | out_neg | out_pos
        rc = step_fn(
            fn, m, ent.data_ptr(), ent.shape[0], ent.stride(0), rel.data_ptr(), rel.shape[0], rel.stride(0),
            model._rel_off, pos.data_ptr(), neg.data_ptr(), neg.stride(0), B, N, model._D, model._gamma_f,
            model._range_f, temp, int(adv), 1, None if w is None else w.data_ptr(), out[4:].data_ptr(), None,
            out[5:].data_ptr(), out[5 + B:].data_ptr(),
            optimizer.state[ent]["exp_avg"].data_ptr(), optimizer.state[ent]["exp_avg_sq"].data_ptr(),
            optimizer.state[rel]["exp_avg"].data_ptr(), optimizer.state[rel]["exp_avg_sq"].data_ptr(),
            float(lr), float(b1), float(b2), float(group["eps"]), int(step), int(group["semantics"] == "keras"),
            ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream,
            *((out.data_ptr(),) if lazy else (reg, out.data_ptr())))
        _lib.check(rc, name)
        model._adam_commit(optimizer, [ent, rel])
        loss, pos_loss, neg_loss, reg_term = out[:4].tolist()
        log = {"regularization": reg_term} if reg != 0.0 else {}
        log.update(positive_sample_loss=pos_loss, negative_sample_loss=neg_loss, loss=loss)
        return log


def _lazy_group(optimizer):
    """Whether the optimizer's group asks for the lazy Adam (optim.Adam(..., lazy=True))."""
    return bool(optimizer.param_groups[0].get("lazy", False))


def default_hidden_range(gamma, hidden_dim, epsilon=2.0):
    """(gamma + epsilon) / hidden_dim (model.py:62,86)."""
    return (gamma + epsilon) / hidden_dim


__all__ = ["TFKGEModel", "KGEModel", "default_hidden_range"]
