"""Mixtral-class MoE decoder.

Same attention stack as llama; the MLP is a top-k routed mixture of SwiGLU
experts.  Experts are TP-sharded on the intermediate dimension (every rank
holds a slice of every expert), so the only collective per MoE block is the
same single all-reduce a dense row-parallel MLP needs — the right trade at
xGMI's per-link bandwidth for the TP=4 baseline config.  Expert compute runs
through the grouped-GEMM HIP kernel (kernels/moe_gemm.hip): tokens sorted by
expert, one fused gate/up+SiLU launch plus one down launch covering every
expert segment — shape-static, so MoE decode steps hipGraph-capture; a
per-expert torch loop remains as the fallback for non-128-aligned dims.
Routing, the sort bookkeeping, the activation gather and the weighted combine
around those two launches are HIP as well (kernels/moe_dispatch.hip), which
makes the TP-sharded block four launches after the router GEMM (five above
256 tokens, where the dispatch takes two).
"""

from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..engine.config import ModelConfig
from ..parallel import divide, get_tp_world_size, tp_all_reduce
from ..parallel.layers import ParallelLMHead, VocabParallelEmbedding, _init_weight
from .llama import Attention, RMSNorm


class MoEBlock(nn.Module):
    def __init__(self, cfg: ModelConfig):
        super().__init__()
        tp = get_tp_world_size()
        self.num_experts = cfg.num_experts
        self.top_k = cfg.num_experts_per_tok
        self.hidden = cfg.hidden_size
        # expert-parallel (E16): whole experts distributed across ranks with
        # token all-to-all; otherwise every rank holds an intermediate slice
        # of every expert (TP-sharded, graph-capturable)
        self.ep = bool(cfg.expert_parallel) and tp > 1 and cfg.num_experts % tp == 0
        if self.ep:
            from ..parallel import get_tp_rank

            self.tp = tp
            self.experts_per_rank = cfg.num_experts // tp
            self.expert0 = get_tp_rank() * self.experts_per_rank
            self.inter = cfg.intermediate_size  # full intermediate
            n_local = self.experts_per_rank
        else:
            self.inter = divide(cfg.intermediate_size, tp)
            n_local = cfg.num_experts
        self.gate = _init_weight((cfg.num_experts, cfg.hidden_size), cfg.dtype, std=0.02)
        # w13: [E_local, 2*I_local, H] fused gate+up; w2: [E_local, H, I_local]
        self.w13 = _init_weight((n_local, 2 * self.inter, cfg.hidden_size), cfg.dtype)
        self.w2 = _init_weight((n_local, cfg.hidden_size, self.inter), cfg.dtype)
        self.quant_bits: int | None = None  # set by quantize_()

    def quantize_(self, qbits: int) -> bool:
        """Replace the bf16 expert weights with RTN-quantized storage (E18):
        buffers w13_q / w13_scale / w2_q / w2_scale in ops.quantize_weight's
        format stacked per expert.  int4 groups scales over 128 k, so a block
        whose hidden or local intermediate size is no multiple of 128 stays
        bf16 (returns False).  The router gate stays bf16."""
        if qbits == 4 and (self.hidden % 128 or self.inter % 128):
            return False
        for name in ("w13", "w2"):
            w = getattr(self, name).data
            # one expert at a time: the f32 working set stays one expert wide
            packed = [ops.quantize_weight(w[e], qbits) for e in range(w.shape[0])]
            delattr(self, name)
            self.register_buffer(name + "_q", torch.stack([q for q, _ in packed]))
            self.register_buffer(name + "_scale", torch.stack([s for _, s in packed]))
        self.quant_bits = qbits
        return True

    def _grouped(self, x, name: str, seg, gated: bool, rows=None):
        """ops.moe_gemm on w13 / w2, packed or bf16."""
        if self.quant_bits is None:
            return ops.moe_gemm(x, getattr(self, name), seg, gated=gated, rows=rows)
        return ops.moe_gemm(x, getattr(self, name + "_q"), seg, gated=gated,
                            rows=rows, scales=getattr(self, name + "_scale"),
                            qbits=self.quant_bits)

    def _expert(self, name: str, e: int, dtype: torch.dtype) -> torch.Tensor:
        """One expert's w13 / w2 for the per-expert loops, dequantised on use."""
        if self.quant_bits is None:
            return getattr(self, name)[e]
        return ops.dequantize_weight(getattr(self, name + "_q")[e],
                                     getattr(self, name + "_scale")[e],
                                     self.quant_bits, dtype)

    def _forward_ep(self, x: torch.Tensor, flat_ids, flat_w, token_idx):
        """Dispatch token copies to their experts' owner ranks (all-to-all),
        compute locally at full intermediate width, return and combine.
        No output all-reduce: each token's k contributions come home and sum
        locally.  Variable split sizes host-sync, so EP runs eager."""
        import torch.distributed as dist

        epr = self.experts_per_rank
        owner = torch.div(flat_ids, epr, rounding_mode="floor")
        send_order = torch.argsort(owner, stable=True)
        send_counts = torch.bincount(owner, minlength=self.tp)
        recv_counts = torch.empty_like(send_counts)
        dist.all_to_all_single(recv_counts, send_counts)
        send_sizes = send_counts.tolist()
        recv_sizes = recv_counts.tolist()

        x_send = x[token_idx[send_order]].contiguous()
        ids_send = flat_ids[send_order].contiguous()
        x_recv = x.new_empty((sum(recv_sizes), self.hidden))
        ids_recv = ids_send.new_empty(sum(recv_sizes))
        dist.all_to_all_single(x_recv, x_send, recv_sizes, send_sizes)
        dist.all_to_all_single(ids_recv, ids_send, recv_sizes, send_sizes)

        local_e = ids_recv - self.expert0
        order2 = torch.argsort(local_e, stable=True)
        xs = x_recv[order2].contiguous()
        if ops.moe_gemm_usable(xs, self.hidden, self.inter):
            counts = torch.zeros(epr, dtype=torch.int32, device=x.device)
            counts.scatter_add_(
                0, local_e, torch.ones_like(local_e, dtype=torch.int32))
            seg = torch.zeros(epr + 1, dtype=torch.int32, device=x.device)
            seg[1:] = counts.cumsum(0).to(torch.int32)
            h = self._grouped(xs, "w13", seg, gated=True)
            ye_sorted = self._grouped(h, "w2", seg, gated=False)
        else:
            ye_sorted = torch.empty_like(xs)
            sorted_e = local_e[order2]
            for e in range(epr):
                sel = (sorted_e == e).nonzero(as_tuple=True)[0]
                h = ops.silu_and_mul(
                    F.linear(xs[sel], self._expert("w13", e, x.dtype)))
                ye_sorted[sel] = F.linear(h, self._expert("w2", e, x.dtype))
        ye = torch.empty_like(ye_sorted)
        ye[order2] = ye_sorted

        y_home = x.new_empty((sum(send_sizes), self.hidden))
        dist.all_to_all_single(y_home, ye.contiguous(), send_sizes, recv_sizes)
        out = torch.zeros_like(x)
        out.index_add_(0, token_idx[send_order],
                       y_home * flat_w[send_order, None])
        return out

    def forward(self, x: torch.Tensor) -> torch.Tensor:  # [T, H]
        t = x.shape[0]
        router_logits = F.linear(x, self.gate)           # [T, E]
        if (not self.ep and t > 0
                and os.environ.get("VTA_MOE_FUSED", "1") != "0"
                and ops.moe_gemm_usable(x, self.hidden, self.inter)
                and ops.moe_dispatch_usable(router_logits, self.top_k)):
            # fused chain (E16): route + dispatch, a gated grouped GEMM that
            # gathers its own rows, the down grouped GEMM, an f32 combine.
            # Launch only, shapes depend on T alone, so it still captures.
            # VTA_MOE_FUSED=0 (read per call) keeps the torch chain below.
            weights, _, seg, src_row, pos = ops.moe_dispatch(
                router_logits, self.top_k)
            h = self._grouped(x, "w13", seg, gated=True, rows=src_row)
            ye = self._grouped(h, "w2", seg, gated=False)
            return tp_all_reduce(ops.moe_combine(ye, pos, weights))
        weights, ids = ops.topk_softmax(router_logits, self.top_k)  # [T, k]
        out = torch.zeros_like(x)
        flat_ids = ids.reshape(-1)                        # [T*k]
        flat_w = weights.reshape(-1).to(x.dtype)
        token_idx = torch.arange(t, device=x.device).repeat_interleave(self.top_k)
        if self.ep:
            return self._forward_ep(x, flat_ids, flat_w, token_idx)
        if ops.moe_gemm_usable(x, self.hidden, self.inter):
            # grouped-GEMM path (E16): sort token-expert pairs by expert and
            # run ONE gated launch + ONE down launch over all segments
            sort_idx = torch.argsort(flat_ids)
            rows = token_idx[sort_idx]
            # capture-safe histogram (torch.bincount host-syncs on its input)
            counts = torch.zeros(self.num_experts, dtype=torch.int32, device=x.device)
            counts.scatter_add_(
                0, flat_ids, torch.ones_like(flat_ids, dtype=torch.int32))
            seg = torch.zeros(self.num_experts + 1, dtype=torch.int32, device=x.device)
            seg[1:] = counts.cumsum(0).to(torch.int32)
            xs = x[rows].contiguous()
            h = self._grouped(xs, "w13", seg, gated=True)
            ye = self._grouped(h, "w2", seg, gated=False)
            out.index_add_(0, rows, ye * flat_w[sort_idx, None])
            return tp_all_reduce(out)
        # Launch-only expert loop: no data-dependent host branches (`any()`
        # would sync per expert and break hipGraph capture); empty selections
        # run zero-row GEMMs, which are free.
        for e in range(self.num_experts):
            sel = (flat_ids == e).nonzero(as_tuple=True)[0]
            rows = token_idx[sel]
            xe = x[rows]
            h = ops.silu_and_mul(F.linear(xe, self._expert("w13", e, x.dtype)))
            ye = F.linear(h, self._expert("w2", e, x.dtype))
            out.index_add_(0, rows, ye * flat_w[sel, None])
        return tp_all_reduce(out)


class MixtralDecoderLayer(nn.Module):
    def __init__(self, cfg: ModelConfig, layer_idx: int):
        super().__init__()
        self.input_norm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps, cfg.dtype)
        self.attn = Attention(cfg, layer_idx)
        self.post_norm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps, cfg.dtype)
        self.moe = MoEBlock(cfg)

    def forward(self, hidden, residual, positions, kv_cache, meta, cos_sin_cache):
        if residual is None:
            residual = hidden
            hidden = self.input_norm(hidden)
        else:
            hidden, residual = self.input_norm(hidden, residual)
        hidden = self.attn(hidden, positions, kv_cache, meta, cos_sin_cache)
        hidden, residual = self.post_norm(hidden, residual)
        hidden = self.moe(hidden)
        return hidden, residual


class MixtralForCausalLM(nn.Module):
    def __init__(self, cfg: ModelConfig):
        super().__init__()
        self.cfg = cfg
        self.embed = VocabParallelEmbedding(cfg.vocab_size, cfg.hidden_size, dtype=cfg.dtype)
        self.layers = nn.ModuleList(
            [MixtralDecoderLayer(cfg, i) for i in range(cfg.num_layers)]
        )
        self.final_norm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps, cfg.dtype)
        self.lm_head = ParallelLMHead(cfg.vocab_size, cfg.hidden_size, dtype=cfg.dtype)
        if cfg.tie_word_embeddings:
            self.lm_head.tie_to(self.embed)
        self.register_buffer(
            "cos_sin_cache",
            ops.make_cos_sin_cache(
                cfg.head_dim, cfg.max_model_len, cfg.rope_theta, cfg.dtype,
                cfg.rope_scaling,
            ),
            persistent=False,
        )

    def forward(self, input_ids, positions, kv_caches, meta):
        hidden = self.embed(input_ids)
        residual = None
        for i, layer in enumerate(self.layers):
            hidden, residual = layer(
                hidden, residual, positions, kv_caches[i], meta, self.cos_sin_cache
            )
        hidden, _ = self.final_norm(hidden, residual)
        return hidden

    def compute_logits(self, hidden: torch.Tensor) -> torch.Tensor:
        return self.lm_head(hidden)

    # ------------------------------------------------------------------
    def load_weights(self, weights: dict[str, torch.Tensor]) -> None:
        """Load an HF-layout Mixtral state dict (TP-aware slicing).

        HF names: block_sparse_moe.experts.E.{w1,w2,w3} = gate/down/up,
        block_sparse_moe.gate = router (reference model family parity).
        """
        from ..parallel import get_tp_rank

        r = get_tp_rank()
        for i, layer in enumerate(self.layers):
            p = f"model.layers.{i}."
            layer.attn.qkv_proj.load_full_weights([
                weights[p + "self_attn.q_proj.weight"],
                weights[p + "self_attn.k_proj.weight"],
                weights[p + "self_attn.v_proj.weight"],
            ])
            layer.attn.o_proj.load_full_weight(weights[p + "self_attn.o_proj.weight"])
            moe = layer.moe
            moe.gate.data.copy_(
                weights[p + "block_sparse_moe.gate.weight"].to(moe.gate.dtype))
            if moe.ep:
                # expert-parallel: this rank holds whole experts
                for le in range(moe.experts_per_rank):
                    e = moe.expert0 + le
                    ep = f"{p}block_sparse_moe.experts.{e}."
                    moe.w13.data[le, :moe.inter].copy_(
                        weights[ep + "w1.weight"].to(moe.w13.dtype))
                    moe.w13.data[le, moe.inter:].copy_(
                        weights[ep + "w3.weight"].to(moe.w13.dtype))
                    moe.w2.data[le].copy_(
                        weights[ep + "w2.weight"].to(moe.w2.dtype))
            else:
                for e in range(moe.num_experts):
                    ep = f"{p}block_sparse_moe.experts.{e}."
                    w1 = weights[ep + "w1.weight"]  # gate [I, H]
                    w3 = weights[ep + "w3.weight"]  # up   [I, H]
                    w2 = weights[ep + "w2.weight"]  # down [H, I]
                    sl = slice(r * moe.inter, (r + 1) * moe.inter)
                    moe.w13.data[e, :moe.inter].copy_(w1[sl].to(moe.w13.dtype))
                    moe.w13.data[e, moe.inter:].copy_(w3[sl].to(moe.w13.dtype))
                    moe.w2.data[e].copy_(w2[:, sl].to(moe.w2.dtype))
            layer.input_norm.weight.data.copy_(
                weights[p + "input_layernorm.weight"].to(self.cfg.dtype))
            layer.post_norm.weight.data.copy_(
                weights[p + "post_attention_layernorm.weight"].to(self.cfg.dtype))
        self.embed.load_full_weight(weights["model.embed_tokens.weight"])
        self.final_norm.weight.data.copy_(weights["model.norm.weight"].to(self.cfg.dtype))
        if not self.cfg.tie_word_embeddings and "lm_head.weight" in weights:
            self.lm_head.load_full_weight(weights["lm_head.weight"])
