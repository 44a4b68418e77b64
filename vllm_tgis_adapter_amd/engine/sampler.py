"""Sampling pipeline.

Per-request temperature / top-k / top-p / seeded RNG / repetition penalty /
min-tokens EOS suppression / logits processors / logprob+rank+top-N
extraction, vectorised over the step's sampling rows.  All tensor math runs
on-device; the per-position logprob dicts the TGIS wire format needs
(grpc_server.py:701-756) are assembled host-side from one batched top-k.

Greedy and plain temperature-sampling rows take the fused HIP kernel
(kernels/sampling.hip, exponential-race identity) in one pass; batches with
top-k/top-p rows take its radix-select sibling
(kernels/sampling_topk_topp.hip) when the logits are bf16/f16 on the GPU.
Repetition-penalty and guided rows stay on those kernels too: their token
sets (seen in prompt + output, allowed by the automaton) are device bitmaps,
1 bit per vocab entry, and kernels/logits_edit.hip edits the logits in place
from them before the sampler and the deferred logprob kernel read them — no
host sync, so the pipelined step keeps overlapping.  Logits processors, and
penalties / guided masks / top-k/top-p over CPU logits (top-k/top-p over f32
too), run the vectorised torch path.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from .request import Request
from .types import Logprob, PosLogprobs

_NEG_INF = float("-inf")

import os as _os_mod

# deferred (async) logprob extraction on the fused path; VTA_DEFER_LP=0
# falls back to the synchronous slow-path extraction
_DEFER_LP = _os_mod.environ.get("VTA_DEFER_LP", "1") == "1"

# slots the seen-bitmap pool doubles up to before it evicts (16 KB each at
# V = 128256); a batch with more penalised rows than this still grows it
_SEEN_POOL_CAP = 1024


@dataclass
class SamplerOutput:
    token_ids: list[int]
    # per sampling row: logprob info for the sampled token (or None)
    logprobs: list[Optional[PosLogprobs]]


def _apply_top_k_top_p(logits: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor) -> torch.Tensor:
    """Mask logits outside top-k / nucleus top-p, rows vectorised."""
    vocab = logits.shape[-1]
    sorted_logits, sorted_idx = torch.sort(logits, dim=-1, descending=True)
    # top-k mask
    ranks = torch.arange(vocab, device=logits.device).unsqueeze(0)
    k = top_k.clamp(min=1, max=vocab).unsqueeze(1)
    mask = ranks >= k
    # top-p mask on the sorted probabilities
    probs = torch.softmax(sorted_logits, dim=-1)
    cum = probs.cumsum(dim=-1)
    pmask = (cum - probs) > top_p.unsqueeze(1)  # keep tokens whose prefix-mass < p
    mask |= pmask
    mask[:, 0] = False  # always keep the argmax token
    sorted_logits = sorted_logits.masked_fill(mask, _NEG_INF)
    return torch.full_like(logits, _NEG_INF).scatter_(-1, sorted_idx, sorted_logits)


class Sampler:
    def __init__(self, device: str, max_logprobs: int = 11):
        self.device = device
        self.max_logprobs = max_logprobs
        # pinned staging (double-buffered): pageable host->device uploads are
        # silently synchronous and would stall the pipelined step's launch
        self._pin: dict = {}
        self._pin_flip = 0
        self._pending_lp = None  # deferred logprob tensors (finish_fused)
        # seen-token bitmaps of penalised requests (logits_edit): device pool
        # int32 [slots, W]; entry = [request, all_token_ids scattered so far,
        # last-used tick] per slot, id(request) -> slot for the lookup
        self._seen: Optional[torch.Tensor] = None
        self._seen_entries: list = []
        self._seen_free: list[int] = []
        self._seen_of: dict[int, int] = {}
        self._seen_tick = 0

    def _h2d_array(self, name: str, arr) -> torch.Tensor:
        """_h2d_list for a numpy array: one pinned staging copy, async upload."""
        src = torch.from_numpy(arr)
        if self.device != "cuda":
            return src
        n = src.numel()
        key = f"{name}.{self._pin_flip}"
        buf = self._pin.get(key)
        if buf is None or buf.numel() < n:
            buf = torch.empty(max(n, 256), dtype=src.dtype, pin_memory=True)
            self._pin[key] = buf
        staging = buf[:n].view(src.shape)
        staging.copy_(src)
        return staging.to(self.device, non_blocking=True)

    def _grow_seen_pool(self, cap: int, words: int, device) -> None:
        old = self._seen
        have = 0 if old is None else old.shape[0]
        pool = torch.zeros((cap, words), dtype=torch.int32, device=device)
        if have:
            pool[:have].copy_(old)
        self._seen = pool
        self._seen_entries.extend([None] * (cap - have))
        self._seen_free.extend(range(cap - 1, have - 1, -1))

    def _alloc_seen_slot(self, in_batch: set) -> int:
        """A free slot; at the pool's cap the least-recently-used slot whose
        request is not in this batch; else a slot of the doubled pool."""
        if not self._seen_free:
            ents = self._seen_entries
            victim = None
            if len(ents) >= _SEEN_POOL_CAP:
                for s, ent in enumerate(ents):
                    if id(ent[0]) not in in_batch and (
                            victim is None or ent[2] < ents[victim][2]):
                        victim = s
            if victim is not None:
                del self._seen_of[id(ents[victim][0])]
                ents[victim] = None
                return victim
            self._grow_seen_pool(2 * len(ents), self._seen.shape[1],
                                 self._seen.device)
        return self._seen_free.pop()

    def _update_seen_pool(
        self, logits: torch.Tensor, requests: list[Request],
        pen_rows: list[int],
    ) -> dict[int, int]:
        """Bring the seen bitmap of every penalised row up to date with its
        request's prompt + output tokens: newly assigned (or rewound) slots
        are zeroed and all rows' new (slot, token) pairs go up in one copy and
        one scatter launch.  Returns row -> slot.  A slot belongs to a Request
        OBJECT (ids are reused); preemption or an abort only leaves a slot
        stale until it is evicted."""
        import numpy as np

        from .. import ops as _ops

        vocab = logits.shape[1]
        words = _ops.token_bitmap_words(vocab)
        if (self._seen is None or self._seen.shape[1] != words
                or self._seen.device != logits.device):
            self._seen = None
            self._seen_entries, self._seen_free, self._seen_of = [], [], {}
            cap = 64
            while cap < len(pen_rows):
                cap *= 2
            self._grow_seen_pool(cap, words, logits.device)
        self._seen_tick += 1
        ents = self._seen_entries
        in_batch = {id(r) for r in requests}
        fresh: list[int] = []
        pair_slots: list[int] = []
        pair_toks: list[int] = []
        slot_of_row: dict[int, int] = {}
        for i in pen_rows:
            req = requests[i]
            n_prompt = len(req.prompt_token_ids)
            n_all = n_prompt + len(req.output_token_ids)
            slot = self._seen_of.get(id(req))
            ent = ents[slot] if slot is not None else None
            if ent is None or ent[0] is not req:
                slot = self._alloc_seen_slot(in_batch)
                ents = self._seen_entries
                ent = ents[slot] = [req, 0, 0]
                self._seen_of[id(req)] = slot
                fresh.append(slot)
            elif n_all < ent[1]:  # history shrank: rebuild from scratch
                ent[1] = 0
                fresh.append(slot)
            upto = ent[1]
            if upto >= n_prompt:  # the steady state: one new output token
                new = req.output_token_ids[upto - n_prompt:]
            else:
                new = req.prompt_token_ids[upto:] + req.output_token_ids
            pair_slots.extend([slot] * len(new))
            pair_toks.extend(new)
            ent[1] = n_all
            ent[2] = self._seen_tick
            slot_of_row[i] = slot
        if fresh:
            # index_fill_ on the slot axis stays asynchronous (see `ban`)
            self._seen.index_fill_(
                0, self._h2d_list("seen_fresh", fresh, torch.long), 0)
        if pair_toks:
            pairs = self._h2d_array(
                "seen_pairs", np.array([pair_slots, pair_toks], dtype=np.int32))
            _ops.token_bitmap_scatter(self._seen, pairs[0], pairs[1], vocab)
        return slot_of_row

    def _launch_logits_edit(
        self, logits: torch.Tensor, requests: list[Request],
        edit_rows: list[int],
    ) -> None:
        """Repetition penalty and guided masks of ``edit_rows`` applied to
        ``logits`` in place by ops.logits_edit, without a host sync: seen
        bitmaps from the per-sampler pool, allow bitmaps packed once per
        automaton state and uploaded as one [G, W] copy."""
        import numpy as np

        from .. import ops as _ops

        vocab = logits.shape[1]
        pen_rows = [i for i in edit_rows
                    if requests[i].sampling_params.repetition_penalty != 1.0]
        seen_slot = (self._update_seen_pool(logits, requests, pen_rows)
                     if pen_rows else {})
        allow_rows: list = []
        # one upload: rows, penalties (f32 bits), seen slots, allow slots
        meta = np.empty((4, len(edit_rows)), dtype=np.int32)
        pens = meta[1].view(np.float32)
        for j, i in enumerate(edit_rows):
            req = requests[i]
            packed = None
            gs = req.guided_state
            if gs is not None:
                pack = getattr(gs, "allowed_bitmap", None)
                if pack is not None:
                    packed = pack(vocab)
                else:
                    ids = gs.allowed_token_ids()
                    if ids is not None:
                        packed = _ops.pack_token_bitmap(ids, vocab)
            meta[0, j] = i
            pens[j] = req.sampling_params.repetition_penalty
            meta[2, j] = seen_slot.get(i, -1)
            meta[3, j] = -1 if packed is None else len(allow_rows)
            if packed is not None:
                allow_rows.append(packed)
        dmeta = self._h2d_array("edit_meta", meta)
        allow = None
        if allow_rows:
            allow = self._h2d_array(
                "edit_allow", np.stack(allow_rows).view(np.int32))
        _ops.logits_edit(
            logits, dmeta[0], dmeta[1].view(torch.float32),
            self._seen if pen_rows else None, dmeta[2], allow, dmeta[3])

    def _h2d_list(self, name: str, data: list, dtype: torch.dtype) -> torch.Tensor:
        if self.device != "cuda":
            return torch.tensor(data, dtype=dtype)
        n = len(data)
        key = f"{name}.{self._pin_flip}"
        buf = self._pin.get(key)
        if buf is None or buf.numel() < n:
            buf = torch.empty(max(n, 256), dtype=dtype, pin_memory=True)
            self._pin[key] = buf
        staging = buf[:n]
        staging.copy_(torch.tensor(data, dtype=dtype))
        return staging.to(self.device, non_blocking=True)

    def _generator_for(self, req: Request) -> Optional[torch.Generator]:
        if req.sampling_params.seed is None:
            return None
        if req.generator is None:
            g = torch.Generator(device=self.device)
            g.manual_seed(req.sampling_params.seed)
            req.generator = g
        return req.generator

    @torch.inference_mode()
    def try_launch_fused(
        self, logits: torch.Tensor, requests: list[Request]
    ) -> Optional[torch.Tensor]:
        """Launch the fused one-pass sampler WITHOUT host sync.

        Returns the device token-id tensor (caller syncs via .tolist()) when
        every row is greedy, plain temperature, or top-k/top-p sampling with
        no logits processors, else None.  Repetition-penalty and guided
        rows qualify where ops.logits_edit_usable holds (GPU logits,
        V % 8 == 0, VTA_SAMPLE_EDIT != 0): their edits are launched here,
        after the EOS ban and before the sampler, from device bitmaps.
        Top-k/top-p
        rows qualify only where the fused HIP sampler serves the logits
        (bf16/f16 on the GPU); on CPU, under VTA_FORCE_REFERENCE, or with
        f32 logits such a batch returns None as before.  Rows that
        request logprobs/top-N stay ON this path: their log-softmax / top-k
        / rank tensors are launched asynchronously here and synced later in
        ``finish_fused`` (the TGIS wire always wants top-N details, and
        dropping to the sync path would stall the pipelined step).  The
        pipelined engine step uses this to overlap host postprocessing with
        the next step's GPU work.
        """
        from .. import ops as _ops

        n, vocab = logits.shape
        simple = True
        any_sampling = False
        any_filter = False  # some sampling row sets top-k / top-p
        filter_ok = _ops.sample_topk_topp_usable(logits)
        edit_ok = _ops.logits_edit_usable(logits)
        ban_rows: list[int] = []  # rows with min_tokens pending: EOS banned
        ban_eos: list[int] = []
        lp_rows: list[int] = []   # rows that want logprob details (deferred)
        edit_rows: list[int] = []  # penalty / guided rows (logits_edit)
        for i, req in enumerate(requests):
            p = req.sampling_params
            if p.logits_processors:
                simple = False
                break
            if p.repetition_penalty != 1.0 or req.guided_state is not None:
                if not edit_ok:  # CPU / force-reference / VTA_SAMPLE_EDIT=0
                    simple = False
                    break
                edit_rows.append(i)
            if p.logprobs is not None:
                if not _DEFER_LP:  # kill switch: old behavior = slow path
                    simple = False
                    break
                lp_rows.append(i)
            if (p.min_tokens and req.num_output_tokens < p.min_tokens
                    and req.eos_token_id is not None):
                ban_rows.append(i)
                ban_eos.append(req.eos_token_id)
            if p.temperature != 0.0:
                any_sampling = True
                if not (p.top_k <= 0 or p.top_k >= vocab) or p.top_p < 1.0:
                    if not filter_ok:  # CPU / force-reference / f32 logits
                        simple = False
                        break
                    any_filter = True
        if not simple:
            self._pending_lp = None
            return None
        import os as _os
        import time as _time

        _dbg = _os.environ.get("VTA_LAUNCH_TIMING", "0") == "1"
        if _dbg:
            _ta = _time.perf_counter()
        self._pin_flip ^= 1
        if ban_rows:
            # min_tokens EOS suppression as ONE batched index_fill_ so the
            # whole batch stays on the fused path.  NOTE: advanced-index
            # assignment (index_put_) host-synchronizes on ROCm — it cost a
            # full hidden GPU-step stall in the pipelined launch phase;
            # flat index_fill_ stays asynchronous.
            flat = [r * vocab + e for r, e in zip(ban_rows, ban_eos)]
            logits.view(-1).index_fill_(
                0, self._h2d_list("ban", flat, torch.long), _NEG_INF)
        if edit_rows:
            self._launch_logits_edit(logits, requests, edit_rows)
        if not _ops.native_enabled(logits):
            # CPU / force-reference: plain argmax-or-race, still deferred-sync
            if not any_sampling:
                out = torch.argmax(logits, dim=-1)
            else:
                probs = torch.softmax(
                    logits.float() / torch.tensor(
                        [max(r.sampling_params.temperature, 1e-6)
                         for r in requests]
                    ).unsqueeze(1),
                    dim=-1,
                )
                q = torch.empty_like(probs)
                for i, req in enumerate(requests):
                    g = self._generator_for(req)
                    if g is None:
                        q[i].exponential_()
                    else:
                        q[i].exponential_(generator=g)
                out = torch.argmax(probs / q, dim=-1)
            self._launch_deferred_logprobs(logits, out, lp_rows, requests)
            return out
        temps = self._h2d_list(
            "temps", [r.sampling_params.temperature for r in requests],
            torch.float32,
        )
        noise = None
        if any_sampling:
            noise = torch.empty((n, vocab), dtype=torch.float32, device=logits.device)
            for i, req in enumerate(requests):
                if req.sampling_params.temperature != 0.0:
                    g = self._generator_for(req)
                    if g is None:
                        noise[i].exponential_()
                    else:
                        noise[i].exponential_(generator=g)
        if _dbg:
            _tb2 = _time.perf_counter()
        out = torch.empty(n, dtype=torch.long, device=logits.device)
        if _dbg:
            _tc = _time.perf_counter()
        if any_filter:
            top_k = self._h2d_list(
                "top_k",
                [min(max(r.sampling_params.top_k, 0), vocab) for r in requests],
                torch.int32,
            )
            top_p = self._h2d_list(
                "top_p", [r.sampling_params.top_p for r in requests],
                torch.float32,
            )
            _ops.sample_topk_topp(out, logits, temps, noise, top_k, top_p)
        else:
            _ops.sample_argmax(out, logits, temps, noise)
        if _dbg:
            _td = _time.perf_counter()
            d = self.__dict__.setdefault("_lt2", [0.0, 0.0, 0.0, 0])
            d[0] += _tb2 - _ta
            d[1] += _tc - _tb2
            d[2] += _td - _tc
            d[3] += 1
            if d[3] >= 128:
                import sys as _sys

                print(f"[sampler-timing] per-step ms ban+temps={d[0]/d[3]*1e3:.2f} "
                      f"empty={d[1]/d[3]*1e3:.2f} kernel-launch={d[2]/d[3]*1e3:.2f}",
                      file=_sys.stderr, flush=True)
                self._lt2 = [0.0, 0.0, 0.0, 0]
        self._launch_deferred_logprobs(logits, out, lp_rows, requests)
        return out

    def _launch_deferred_logprobs(
        self, logits: torch.Tensor, out: torch.Tensor,
        lp_rows: list[int], requests: list[Request],
    ) -> None:
        """Launch log-softmax/top-k/rank work for logprob rows WITHOUT a
        host sync; ``finish_fused`` syncs and builds the wire dicts.  Uses
        the post-min_tokens-ban logits — same semantics as the sync path
        (``sample`` bans EOS before its log_softmax too)."""
        self._pending_lp = None
        if not lp_rows:
            return
        from .. import ops as _ops

        n, vocab = logits.shape
        k = min(self.max_logprobs, vocab)
        if len(lp_rows) == n:
            rows = logits
            chosen = out
        else:
            idx = self._h2d_list("lp_rows", lp_rows, torch.long)
            rows = logits.index_select(0, idx)
            chosen = out.index_select(0, idx)
        if _ops.logsoftmax_topk_usable(rows):
            # one-HBM-pass HIP kernel (E8): log-softmax + top-K + rank
            topv, topi, chosen_lp, ranks = _ops.logsoftmax_topk(
                rows, chosen, k)
        else:
            lp = torch.log_softmax(rows.float(), dim=-1)
            topv, topi = torch.topk(lp, k, dim=-1)
            chosen_lp = lp.gather(1, chosen.unsqueeze(1)).squeeze(1)
            ranks = (lp > chosen_lp.unsqueeze(1)).sum(dim=-1) + 1
        self._pending_lp = (
            topv, topi, chosen_lp, ranks, list(lp_rows),
            [requests[i].sampling_params.logprobs for i in lp_rows],
        )

    def finish_fused(self, token_ids: list[int]) -> SamplerOutput:
        """Sync the deferred logprob tensors (if any) and build the
        per-position dicts the wire format needs."""
        out_logprobs: list[Optional[PosLogprobs]] = [None] * len(token_ids)
        pend = getattr(self, "_pending_lp", None)
        self._pending_lp = None
        if pend is not None:
            topv, topi, chosen_lp, ranks, rows_idx, nums = pend
            topv = topv.tolist()
            topi = topi.tolist()
            chosen_lp = chosen_lp.tolist()
            ranks = ranks.tolist()
            for row, i in enumerate(rows_idx):
                d: PosLogprobs = {}
                for j in range(min(nums[row], len(topi[row]))):
                    d[topi[row][j]] = Logprob(logprob=topv[row][j], rank=j + 1)
                tok = token_ids[i]
                if tok not in d:
                    d[tok] = Logprob(logprob=chosen_lp[row], rank=ranks[row])
                out_logprobs[i] = d
        return SamplerOutput(token_ids=token_ids, logprobs=out_logprobs)

    @torch.inference_mode()
    def sample(self, logits: torch.Tensor, requests: list[Request]) -> SamplerOutput:
        """logits: [N, vocab] raw lm-head outputs for the N sampling rows.

        The all-greedy no-extras batch (the serving steady state) stays in
        the lm-head dtype end to end — one argmax pass, no [N, vocab] f32
        materialisation (2x 131 MB per step at batch 256 / 128k vocab).
        """
        n, vocab = logits.shape
        assert n == len(requests)

        fused = self.try_launch_fused(logits, requests)
        if fused is not None:
            return self.finish_fused(fused.tolist())

        logits = logits.float()

        # --- per-request host-side adjustments (rare paths) -------------
        for i, req in enumerate(requests):
            p = req.sampling_params
            # repetition penalty over prompt + generated tokens
            if p.repetition_penalty != 1.0:
                ids = torch.tensor(
                    sorted(set(req.all_token_ids)), device=logits.device, dtype=torch.long
                )
                row = logits[i]
                vals = row[ids]
                row[ids] = torch.where(
                    vals > 0, vals / p.repetition_penalty, vals * p.repetition_penalty
                )
            # custom logits processors (typical_p, length penalty, ...)
            if p.logits_processors:
                row = logits[i]
                for proc in p.logits_processors:
                    row = proc(req.output_token_ids, row)
                logits[i] = row
            # guided decoding token mask
            if req.guided_state is not None:
                allowed = req.guided_state.allowed_token_ids()
                if allowed is not None:
                    mask = torch.full((vocab,), _NEG_INF, device=logits.device)
                    idx = torch.tensor(allowed, device=logits.device, dtype=torch.long)
                    mask[idx] = 0.0
                    logits[i] += mask
            # min_tokens: suppress EOS until satisfied
            if p.min_tokens and req.num_output_tokens < p.min_tokens and req.eos_token_id is not None:
                logits[i, req.eos_token_id] = _NEG_INF

        # --- logprob extraction uses pre-temperature logits --------------
        need_lp = [i for i, r in enumerate(requests) if r.sampling_params.logprobs is not None]
        logprob_rows = torch.log_softmax(logits[need_lp], dim=-1) if need_lp else None

        # --- sampling -----------------------------------------------------
        temps = torch.tensor(
            [r.sampling_params.temperature for r in requests],
            device=logits.device, dtype=torch.float,
        )
        greedy_mask = temps == 0.0
        sampled = torch.empty(n, dtype=torch.long, device=logits.device)

        if bool(greedy_mask.any()):
            sampled[greedy_mask] = torch.argmax(logits[greedy_mask], dim=-1)

        sample_idx = (~greedy_mask).nonzero(as_tuple=True)[0]
        if len(sample_idx):
            sub = logits[sample_idx] / temps[sample_idx].unsqueeze(1)
            top_k = torch.tensor(
                [
                    requests[i].sampling_params.top_k
                    if requests[i].sampling_params.top_k > 0 else vocab
                    for i in sample_idx.tolist()
                ],
                device=logits.device,
            )
            top_p = torch.tensor(
                [requests[i].sampling_params.top_p for i in sample_idx.tolist()],
                device=logits.device, dtype=torch.float,
            )
            if bool((top_k < vocab).any()) or bool((top_p < 1.0).any()):
                sub = _apply_top_k_top_p(sub, top_k, top_p)
            probs = torch.softmax(sub, dim=-1)
            # exponential-race sampling; per-request generator when seeded
            q = torch.empty_like(probs)
            rows_with_seed = [
                (j, self._generator_for(requests[i]))
                for j, i in enumerate(sample_idx.tolist())
            ]
            if all(g is None for _, g in rows_with_seed):
                q.exponential_()
            else:
                for j, g in rows_with_seed:
                    q[j].exponential_(generator=g)
            sampled[sample_idx] = torch.argmax(probs / q, dim=-1)

        # --- assemble host results ---------------------------------------
        sampled_cpu = sampled.tolist()
        out_logprobs: list[Optional[PosLogprobs]] = [None] * n
        if need_lp:
            k = self.max_logprobs
            lp = logprob_rows
            chosen = sampled[need_lp]
            chosen_lp = lp.gather(1, chosen.unsqueeze(1)).squeeze(1)
            ranks = (lp > chosen_lp.unsqueeze(1)).sum(dim=-1) + 1
            topv, topi = torch.topk(lp, min(k, vocab), dim=-1)
            topv = topv.tolist()
            topi = topi.tolist()
            chosen_lp = chosen_lp.tolist()
            ranks = ranks.tolist()
            for row, i in enumerate(need_lp):
                req = requests[i]
                num = req.sampling_params.logprobs
                d: PosLogprobs = {}
                for j in range(min(num, len(topi[row]))):
                    d[topi[row][j]] = Logprob(logprob=topv[row][j], rank=j + 1)
                tok = sampled_cpu[i]
                if tok not in d:
                    d[tok] = Logprob(logprob=chosen_lp[row], rank=ranks[row])
                out_logprobs[i] = d
        return SamplerOutput(token_ids=sampled_cpu, logprobs=out_logprobs)


def prompt_logprob_dicts(
    logprob_rows: torch.Tensor,  # [M, vocab] log-softmax rows
    actual_ids: list[int],
    num_logprobs: int,
) -> list[PosLogprobs]:
    """Build per-position logprob dicts for prompt tokens (E8)."""
    m, vocab = logprob_rows.shape
    k = min(max(num_logprobs, 1), vocab)
    topv, topi = torch.topk(logprob_rows, k, dim=-1)
    ids_t = torch.tensor(actual_ids, device=logprob_rows.device, dtype=torch.long)
    actual_lp = logprob_rows.gather(1, ids_t.unsqueeze(1)).squeeze(1)
    ranks = (logprob_rows > actual_lp.unsqueeze(1)).sum(dim=-1) + 1
    topv = topv.tolist()
    topi = topi.tolist()
    actual_lp = actual_lp.tolist()
    ranks = ranks.tolist()
    out = []
    for r in range(m):
        d: PosLogprobs = {}
        for j in range(min(num_logprobs, len(topi[r]))):
            d[topi[r][j]] = Logprob(logprob=topv[r][j], rank=j + 1)
        tok = actual_ids[r]
        if tok not in d:
            d[tok] = Logprob(logprob=actual_lp[r], rank=ranks[r])
        out.append(d)
    return out
