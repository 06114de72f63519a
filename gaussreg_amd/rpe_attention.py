"""Mirror of geotransformer/modules/transformer/rpe_transformer.py:18-72 (RPEMultiHeadAttention) -- inference by default,
with autograd (HIP backward, same source file as the forward: csrc/rpe_attention.hip) inside `gaussreg_amd.kpconv.differentiable()`.

The reference projects the (B,N,M,C) relative-position embedding through `proj_p` in every layer (77 GFLOP and a
602 MB temporary at N=M=767, C=256) before contracting it with q.  The contraction is linear in the embedding, so it
is re-associated here:  s_p[h,n,m] = emb[n,m,:] . (W_p[h]^T q[h,n,:]) + q[h,n,:] . b_p[h], and everything after the four
input projections -- q k^T, the positional term, scaling, factors / weights / masks, softmax and scores @ v -- runs in ONE
HIP kernel per batch element (gaussreg_amd/csrc/rpe_attention.hip: gr_rpe_attention): the embedding is streamed exactly
once per layer and no (H,N,M) or (N,M,C) intermediate goes through HBM.  The projections (nn.Linear) and the tiny
u = W_p^T q product stay torch ops.  State-dict keys are the reference's.

Inside `differentiable()` the same projections run under torch autograd and the same forward kernel runs inside one
autograd Function that keeps the embedding (by reference), u, the projected q / k / v and the probabilities; its backward is
one gr_rpe_attention_backward call per element: a row pass that streams the embedding once more -- for grad_u and, when the
embedding wants a gradient, grad_embed -- and a column pass for the key-side sums.  `attention_factors`, `key_weights` and
masks get no gradient.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .kpconv import differentiable_active, no_grad_unless_differentiable


def _attention_forward(emb, u, add, q2, k2, v2, fac, kw, km, H, scores=None, hidden=None):
    """gr_rpe_attention on the float32 contiguous tensors of one batch element -> hidden (N,C), scores (H,N,M), written into
    the caller's tensors where it passes them."""
    dev = q2.device
    (N, C), M = q2.shape, k2.shape[0]
    scores = torch.empty((H, N, M), dtype=torch.float32, device=dev) if scores is None else scores
    hidden = torch.empty((N, C), dtype=torch.float32, device=dev) if hidden is None else hidden
    _lib.call(dev, "gr_rpe_attention", emb, u, add, q2, k2, v2, fac, kw, km, N, M, C, H, scores, hidden)
    return hidden, scores


class _RPEAttentionFunction(torch.autograd.Function):
    """Forward: the inference kernel.  Backward: gr_rpe_attention_backward.  Saved: the inputs and the probabilities, all by
    reference (the (N,M,C) embedding is the caller's tensor, not a copy)."""

    @staticmethod
    def forward(ctx, emb, u, add, q2, k2, v2, fac, kw, km, H):
        hidden, scores = _attention_forward(emb, u, add, q2, k2, v2, fac, kw, km, H)
        ctx.save_for_backward(emb, u, q2, k2, v2, scores, fac, kw)
        ctx.H = H
        ctx.set_materialize_grads(False)       # an unused output hands over None: the kernel's null grad_scores path
        return hidden, scores

    @staticmethod
    def backward(ctx, grad_hidden, grad_scores):
        emb, u, q2, k2, v2, scores, fac, kw = ctx.saved_tensors
        if grad_hidden is None and grad_scores is None:
            return (None,) * 10
        dev = q2.device
        (N, C), M, H = q2.shape, k2.shape[0], ctx.H
        gh = torch.zeros_like(q2) if grad_hidden is None else grad_hidden.to(torch.float32).contiguous()
        gs = None if grad_scores is None else grad_scores.to(torch.float32).contiguous()
        gq, gk, gv, gu = torch.empty_like(q2), torch.empty_like(k2), torch.empty_like(v2), torch.empty_like(u)
        gadd = torch.empty((N, H), dtype=torch.float32, device=dev)
        gemb = torch.empty_like(emb) if ctx.needs_input_grad[0] else None
        _lib.call(dev, "gr_rpe_attention_backward", emb, u, q2, k2, v2, scores, fac, kw, gh, gs, N, M, C, H, gq, gk, gv, gu,
                  gadd, gemb, ws=_lib.lib().gr_rpe_attention_backward_workspace_bytes(N, M, H))
        return gemb, gu, gadd, gq, gk, gv, None, None, None, None


class RPEMultiHeadAttention(nn.Module):
    def __init__(self, d_model, num_heads, dropout=None):
        super().__init__()
        if d_model % num_heads != 0:
            raise ValueError('`d_model` ({}) must be a multiple of `num_heads` ({}).'.format(d_model, num_heads))
        self.d_model = d_model
        self.num_heads = num_heads
        self.d_model_per_head = d_model // num_heads
        self.proj_q = nn.Linear(self.d_model, self.d_model)
        self.proj_k = nn.Linear(self.d_model, self.d_model)
        self.proj_v = nn.Linear(self.d_model, self.d_model)
        self.proj_p = nn.Linear(self.d_model, self.d_model)
        self.dropout = nn.Identity() if dropout is None or dropout <= 0 else nn.Dropout(dropout)

    @no_grad_unless_differentiable
    def forward(self, input_q, input_k, input_v, embed_qk, key_weights=None, key_masks=None, attention_factors=None,
                lengths=None):
        """(B,N,C), (B,M,C), (B,M,C), (B,N,M,C) -> hidden_states (B,N,C), attention_scores (B,H,N,M).

        `lengths` (not in the reference; a list of B ints, self-attention only): the batch is a padded stack of B clouds of
        different sizes -- element b has lengths[b] real rows, `embed_qk` is then a LIST of B tensors (n_b, n_b, C).  The
        fused kernel runs per element with its true size, so the real rows are exactly what the unpadded call returns;
        padded rows of hidden_states are zero, attention_scores is None.

        Inside `differentiable()` (grad mode on) the outputs carry a grad_fn; their values are those of inference: the same
        projections and the same kernel, the kernel inside _RPEAttentionFunction, everything around it torch ops with their
        own grad.  What the backward could not do is refused here and not at backward()."""
        train = differentiable_active()
        if train:
            for name, t in (("key_weights", key_weights), ("attention_factors", attention_factors)):
                if t is not None and t.requires_grad:
                    raise ValueError(f"{name} requires grad, but the HIP RPE attention has no gradient with respect to it")
            if isinstance(self.dropout, nn.Dropout) and self.training and self.dropout.p > 0:
                raise NotImplementedError("RPEMultiHeadAttention: dropout on the attention scores is not differentiable here")
        _lib.require_gpu()
        if not input_q.is_cuda:
            raise RuntimeError("RPEMultiHeadAttention: inputs must live on the GPU")
        if lengths is not None:
            return self._forward_ragged(input_q, input_k, input_v, embed_qk, lengths, train), None
        dev = input_q.device
        B, N, C = input_q.shape
        M, H = input_k.shape[1], self.num_heads
        emb = embed_qk.to(torch.float32).contiguous()
        fac, kw, km = (None if t is None else t.to(dtype).contiguous() for t, dtype in
                       ((attention_factors, torch.float32), (key_weights, torch.float32), (key_masks, torch.uint8)))

        def element(b, **out):
            # B = 1: a view, whose backward is a view of the (N,M,C) gradient (a select would copy it into zeros)
            return self._attend(input_q[b], input_k[b], input_v[b], emb.view(N, M, C) if B == 1 else emb[b],
                                None if fac is None else fac[b], None if kw is None else kw[b],
                                None if km is None else km[b], **out)

        if train:
            outs = [element(b) for b in range(B)]
            if B == 1:
                return outs[0][0].unsqueeze(0), outs[0][1].unsqueeze(0)
            return torch.stack([hid for hid, _ in outs]), torch.stack([sc for _, sc in outs])
        scores = torch.empty((B, H, N, M), dtype=torch.float32, device=dev)
        hidden = torch.empty((B, N, C), dtype=torch.float32, device=dev)
        for b in range(B):
            element(b, scores=scores[b], hidden=hidden[b])
        if not isinstance(self.dropout, nn.Identity):
            scores = self.dropout(scores)  # inference: identity (the reference applies dropout to the scores before @ v)
        return hidden, scores

    def _forward_ragged(self, input_q, input_k, input_v, embed_list, lengths, train):
        """hidden_states (B,N,C) of a padded stack: element b alone with its lengths[b] rows, zeros below them."""
        dev = input_q.device
        B, N, C = input_q.shape
        if input_k.shape != input_q.shape or len(embed_list) != B or len(lengths) != B:
            raise ValueError("lengths: self-attention over a padded stack, one embedding per element")
        lengths = [int(n) for n in lengths]

        def element(b, **out):
            n, emb = lengths[b], embed_list[b]
            if emb.shape != (n, n, C) or not emb.is_contiguous() or emb.dtype != torch.float32:
                raise ValueError("embedding %d must be a contiguous float32 (n, n, C) tensor" % b)
            if n == 0:
                return None
            return self._attend(input_q[b, :n], input_k[b, :n], input_v[b, :n], emb, None, None, None, **out)

        if train:
            rows = []
            for b in range(B):
                out = element(b)                                                  # hidden and its own scores tensor
                rows.append(torch.zeros((N, C), dtype=torch.float32, device=dev) if out is None
                            else F.pad(out[0], (0, 0, 0, N - lengths[b])))
            return torch.stack(rows)
        hidden = torch.zeros((B, N, C), dtype=torch.float32, device=dev)
        nmax = max(lengths)
        scores = torch.empty((self.num_heads, nmax, nmax), dtype=torch.float32, device=dev)   # scratch: written, never read
        for b in range(B):
            element(b, scores=scores, hidden=hidden[b])
        return hidden

    def _attend(self, xq, xk, xv, emb, fac, kw, km, **out):
        """One batch element: `_project`, then the kernel -- through the autograd Function inside `differentiable()`, else
        straight into `scores=` / `hidden=`.  -> hidden (n,C), scores (H,n,m)."""
        H = self.num_heads
        q2, k2, v2, u, add = self._project(xq, xk, xv)
        if not differentiable_active():
            return _attention_forward(emb, u, add, q2, k2, v2, fac, kw, km, H, **out)
        max_keys = _lib.lib().gr_rpe_attention_backward_max_keys(self.d_model, H)
        if k2.shape[0] > max_keys:
            raise RuntimeError("gaussreg_hip: rpe_attention_backward: %d keys x %d heads do not fit in LDS (at most %d keys "
                               "inside differentiable())" % (k2.shape[0], H, max_keys))
        return _RPEAttentionFunction.apply(emb, u, add, q2, k2, v2, fac, kw, km, H)

    def _project(self, xq, xk, xv):
        """The torch side of ONE batch element, (n,C) / (m,C) / (m,C) matrices: the three input projections (heads side by
        side), u = W_p[h]^T q[h] (n,H,C) and add = q[h] . b_p[h] (n,H).  Per element on purpose: the GEMM a BLAS call runs
        -- and with it the last bit of every product -- follows the operand shapes, nn.Linear included, so projections taken
        over a whole (padded) batch differ from the single call's.  Every element goes through the same calls with the shapes
        it has alone: a batched, a padded and a single call then return the same bits."""
        H, ch, C = self.num_heads, self.d_model_per_head, self.d_model
        q2 = self.proj_q(xq.contiguous()).contiguous()
        k2 = self.proj_k(xk.contiguous()).contiguous()
        v2 = self.proj_v(xv.contiguous()).contiguous()
        qh = q2.view(-1, H, ch)
        u = torch.einsum('nhc,hcj->nhj', qh, self.proj_p.weight.view(H, ch, C)).contiguous()   # rows h*ch..: head h
        add = torch.einsum('nhc,hc->nh', qh, self.proj_p.bias.view(H, ch)).contiguous()
        return q2, k2, v2, u, add
