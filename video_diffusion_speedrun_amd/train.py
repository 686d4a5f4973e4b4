"""Train-step harness with the reference's `train.py::forward` signature (train.py:51-145) and
the loop body of train.py:431-434, on the HIP path.

    total_loss, diffusion_loss = forward(dit_model, batch, text_encoder, tokenizer, device,
                                         global_step, master_process, generator=None, ...)
    optimizer.zero_grad(); total_loss.backward(); optimizer.step(); lr_scheduler.step()

`batch` = {"latent": Tensor[B,C,T,H,W], "prompt": list[str]}; the text encoder is the caller's
(frozen, third-party; out of scope) -- for synthetic runs pass `batch["context"]` (a pre-encoded
[B,Lc,Cc] tensor) and text_encoder=None.  Optional `batch["context_lens"]` ([B] ints: the number of real caption tokens
of each sample, `lens_from_mask(attention_mask)`) restricts the cross-attention to those rows (DiT.forward).

`forward(..., frame_mode="first_frame" | "independent")` trains with one noise level per token-frame (image-to-video
conditioning, diffusion forcing): DiT.forward takes `timesteps [B, t]`, the noising and the loss work per frame.
`frame_mode="chunk"` (a DiT built with frame_chunk=c): one noise level per chunk of c token-frames.
"""
from __future__ import annotations

import logging
from typing import Optional

import torch

from . import ops

bf16, f32 = torch.bfloat16, torch.float32
ALPHA = 8.0  # time shift, train.py:95


def lens_from_mask(attention_mask) -> torch.Tensor:
    """Tokenizer attention mask [B, Lc] (0/1 or bool, right-padded) -> int32 [B] on the CPU: the number of leading ones of
    every row.  A mask with a one after a zero is not a prefix and cannot be expressed as a length: ValueError."""
    m = torch.as_tensor(attention_mask).cpu()
    if m.dim() != 2:
        raise ValueError(f"lens_from_mask: a [B, Lc] mask expected, got shape {tuple(m.shape)}")
    m = m != 0
    lens = m.sum(dim=1)
    prefix = torch.arange(m.shape[1]).unsqueeze(0) < lens.unsqueeze(1)
    if not torch.equal(m, prefix):
        bad = [b for b in range(m.shape[0]) if not torch.equal(m[b], prefix[b])]
        raise ValueError(f"lens_from_mask: the mask of sample(s) {bad} is not a prefix (a one follows a zero)")
    return lens.to(torch.int32)


def encode_prompt_with_t5(text_encoder, tokenizer, max_sequence_length=512, prompt=None, device=None,
                          return_index=-1, return_lengths=False):
    """Caption -> encoder hidden states [B, max_sequence_length, C] in the encoder's dtype, same call contract as
    the reference's helper (utils.py:38-80).  The encoder is the caller's frozen third-party model: host glue only.
    return_lengths=True: (states, lens) with lens = lens_from_mask(the tokenizer's attention_mask), int32 [B] on the CPU."""
    prompts = [prompt] if isinstance(prompt, str) else list(prompt)
    tokens = tokenizer(prompts, padding="max_length", max_length=max_sequence_length, truncation=True,
                       return_length=False, return_overflowing_tokens=False, return_tensors="pt")
    states = text_encoder(tokens.input_ids.to(device), return_dict=True, output_hidden_states=True).hidden_states
    chosen = states[return_index]
    if return_index != -1:  # an inner layer: finish it the way the encoder finishes its last one
        chosen = text_encoder.encoder.dropout(text_encoder.encoder.final_layer_norm(chosen))
    chosen = chosen.to(device=device, dtype=text_encoder.dtype)
    if return_lengths:
        return chosen, lens_from_mask(tokens.attention_mask)
    return chosen


class _FlowLoss(torch.autograd.Function):
    """mean_b mean_{chw} (v - out)^2 in fp32 (train.py:121-125); HIP kernels for value and gradient.  The
    backward honours the upstream gradient (`(loss / n).backward()`, loss scaling): it is read from device
    memory by the kernel, so nothing synchronises and a captured step stays replayable."""

    @staticmethod
    def forward(ctx, out, v):
        loss, per, _ = ops.flow_loss(v, out, want_grad=False)
        ctx.save_for_backward(out, v)
        ctx.mark_non_differentiable(per)
        return loss.reshape(()), per

    @staticmethod
    def backward(ctx, gloss, _gper):
        out, v = ctx.saved_tensors
        return ops.flow_loss_bwd(v, out, gloss.to(f32).reshape(1).contiguous()), None


def flow_loss(out, v):
    return _FlowLoss.apply(out, v)


class _FrameFlowLoss(torch.autograd.Function):
    """frame-weighted flow loss: mean_b sum_f w[b,f] SSE[b,f] / (n_f sum_f w[b,f]) (ops.flow_loss_frames); the upstream
    gradient is read from device memory, as in _FlowLoss.  w gets no gradient."""

    @staticmethod
    def forward(ctx, out, v, w, time_patch):
        loss, per, _ = ops.flow_loss_frames(v, out, w, time_patch, want_grad=False)
        ctx.save_for_backward(out, v, w)
        ctx.time_patch = time_patch
        ctx.mark_non_differentiable(per)
        return loss.reshape(()), per

    @staticmethod
    def backward(ctx, gloss, _gper):
        out, v, w = ctx.saved_tensors
        return ops.flow_loss_frames_bwd(v, out, w, ctx.time_patch, gloss.to(f32).reshape(1).contiguous()), None, None, None


def frame_flow_loss(out, v, weights, time_patch: int):
    """out / v [B,C,T,H,W] bf16, weights f32 [B, T // time_patch] >= 0 -> (loss, per_sample [B]); a sample whose weights
    are all zero contributes 0 and gets a zero gradient"""
    return _FrameFlowLoss.apply(out.contiguous(), v.contiguous(), weights.to(f32).contiguous(), int(time_patch))


FRAME_MODES = (None, "first_frame", "independent", "chunk", "teacher")


def frame_group_of(l: int, n_frames: int, lead: int = 16) -> int:
    """modulation group of token row l of a sample under per-frame timesteps: 0 for the `lead` register rows, then
    1 + the token-frame of the row (token order (h w t), t fastest)"""
    return ops.mod_group_of(l, lead, n_frames)


def _check_chunk(chunk) -> int:
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"frame_mode='chunk': chunk = {chunk!r} must be an int >= 1 (the model's frame_chunk)")
    return chunk


def draw_frame_levels(frame_mode: str, B: int, n_frames: int, device, generator=None, chunk: int = 1) -> torch.Tensor:
    """the first random draw of a per-frame step, in bf16: "first_frame" -> t [B], the very draw of the per-sample path
    (randn(B), time shift); "independent" -> t [B, n_frames], one level per token-frame; "chunk" -> t [B, ceil(n_frames /
    chunk)], one level per chunk of `chunk` token-frames"""
    if frame_mode not in ("first_frame", "independent", "chunk"):
        raise ValueError(f"frame_mode must be one of {FRAME_MODES}, got {frame_mode!r}")
    if frame_mode == "chunk":
        shape = (B, -(-n_frames // _check_chunk(chunk)))
    else:
        shape = (B,) if frame_mode == "first_frame" else (B, n_frames)
    return time_shift_from_normal(torch.randn(shape, device=device, dtype=bf16, generator=generator))


def frame_schedule(frame_mode: str, t: torch.Tensor, n_frames: int, cond_prob: float = 0.5, generator=None,
                   chunk: int = 1):
    """levels from draw_frame_levels -> (timesteps [B, n_frames] in t.dtype, weights f32 [B, n_frames]).
    "first_frame": every frame of sample b at t[b]; with probability cond_prob token-frame 0 is a clean conditioning
    frame -- t = 0 and weight 0 (out of the loss).  "independent": t as drawn, weights 1.  "chunk": t [B, ceil(n_frames /
    chunk)], every level repeated over the `chunk` token-frames of its chunk and cut to n_frames, weights 1.
    Only device-side elementwise work: no host sync, no boolean indexing (capturable)."""
    if frame_mode == "chunk":
        n_chunks = -(-n_frames // _check_chunk(chunk))
        if t.dim() != 2 or t.shape[1] != n_chunks:
            raise ValueError(f"frame_schedule('chunk'): t [B, {n_chunks}] expected (ceil({n_frames} / {chunk}) chunks), got "
                             f"{tuple(t.shape)}")
        tf = t.repeat_interleave(chunk, dim=1)[:, :n_frames].contiguous()
        return tf, torch.ones(tf.shape, dtype=f32, device=t.device)
    if frame_mode == "independent":
        if t.dim() != 2 or t.shape[1] != n_frames:
            raise ValueError(f"frame_schedule('independent'): t [B, {n_frames}] expected, got {tuple(t.shape)}")
        return t, torch.ones(t.shape, dtype=f32, device=t.device)
    if frame_mode != "first_frame":
        raise ValueError(f"frame_mode must be one of {FRAME_MODES}, got {frame_mode!r}")
    if t.dim() != 1:
        raise ValueError(f"frame_schedule('first_frame'): t [B] expected, got {tuple(t.shape)}")
    B = t.shape[0]
    cond = torch.rand(B, device=t.device, generator=generator) < cond_prob
    clean = cond[:, None] & (torch.arange(n_frames, device=t.device) == 0)[None, :]
    tf = torch.where(clean, torch.zeros((), dtype=t.dtype, device=t.device), t[:, None].expand(B, n_frames))
    w = torch.where(clean, torch.zeros((), dtype=f32, device=t.device), torch.ones((), dtype=f32, device=t.device))
    return tf.contiguous(), w.contiguous()


def time_shift_from_normal(z: torch.Tensor) -> torch.Tensor:
    """t = sigmoid(z); t = a t / (1 + (a-1) t), in z.dtype (bf16) like train.py:93-96.
    B scalars: left to torch (host-side plumbing, not a hot-path kernel)."""
    t = torch.sigmoid(z)
    return t * ALPHA / (1 + (ALPHA - 1) * t)


def forward(dit_model, batch, text_encoder, tokenizer, device, global_step, master_process, generator=None,
            binnings=None, batch_size=None, return_index=-1, rope_start=None, frame_mode=None, cond_prob=0.5,
            frame_timesteps=None, frame_weights=None, route=None):
    """frame_mode=None (default): one noise level per sample, the reference's step.
    route: passed to DiT.forward (a model with enable_token_routing routes itself in training mode; this pins the subset
    or, with False, runs the full model).
    frame_mode="first_frame": one level per sample, and with probability cond_prob token-frame 0 stays clean (t = 0) and
    leaves the loss (image-to-video); "independent": one level per token-frame (diffusion forcing); "chunk": one level
    per chunk of the model's frame_chunk token-frames (what a chunk-at-a-time rollout meets), weights 1.
    "teacher": teacher forcing -- the levels are drawn exactly as "chunk" draws them (the same generator draws in the same
    order), and the model runs [registers | clean frames | noisy frames] (DiT.forward(teacher_latents=)): every noisy
    chunk attends the registers at level 1.0, the clean chunks before it and itself, which is what the cached rollout
    computes for that chunk; the loss is taken on the noisy half, weights 1.  frame_timesteps
    [B, t] / frame_weights [B, t] override the drawn levels / weights (t = T // time_patch_size)."""
    logger = logging.getLogger(__name__)
    vae_latent = batch["latent"].to(device).to(bf16)
    with torch.no_grad():
        if "context" in batch and text_encoder is None:
            caption_encoded = batch["context"].to(device)
        else:
            caption_encoded = encode_prompt_with_t5(text_encoder, tokenizer, prompt=batch["prompt"], device=device,
                                                    return_index=return_index)
        caption_encoded = caption_encoded.to(bf16)
        do_zero_out = torch.rand(caption_encoded.shape[0], device=device) < 0.01  # train.py:86
        # same result as `caption_encoded[do_zero_out] = 0` without the host sync of a boolean index
        # (capturable) and without writing into the caller's batch["context"]
        caption_encoded = torch.where(do_zero_out[:, None, None], torch.zeros((), dtype=bf16, device=device),
                                      caption_encoded)
        context_lens = batch.get("context_lens")
        if context_lens is not None:
            # a dropped caption is no context at all: its length goes to 0 as its rows go to zero (on the device: capturable)
            from .model import check_context_lens
            context_lens = check_context_lens(context_lens, caption_encoded.shape[0], caption_encoded.shape[1]).to(device)
            context_lens = torch.where(do_zero_out, torch.zeros((), dtype=torch.int32, device=device), context_lens)
    B = vae_latent.size(0)
    kw = {} if context_lens is None else {"context_lens": context_lens}
    if route is not None:
        kw["route"] = route
    if frame_mode is not None or frame_timesteps is not None or frame_weights is not None:
        # per-frame path.  Draw order: levels, noise, conditioning -- "first_frame" consumes the generator exactly as the
        # per-sample path does for its first two draws
        pt = dit_model.time_patch_size
        n_frames = vae_latent.shape[2] // pt
        teacher = frame_mode == "teacher"
        if teacher:
            if not (getattr(dit_model, "frame_causal", False) and getattr(dit_model, "frame_major", False)) or \
                    getattr(dit_model, "frame_window", None) is not None:
                raise ValueError("frame_mode='teacher' needs a model built with frame_causal=True, frame_major=True and "
                                 "frame_window=None (the teacher-forcing mask); train any other model with "
                                 "frame_mode='chunk' or 'independent'")
            kw = dict(kw, teacher_latents=vae_latent)
        draw_mode = "chunk" if teacher else frame_mode  # teacher: the draws of "chunk", in the same order
        if frame_timesteps is None:
            if frame_mode is None:
                raise ValueError("frame_weights without frame_mode or frame_timesteps: nothing defines the per-frame levels")
            ckw = {"chunk": int(getattr(dit_model, "frame_chunk", 1))} if frame_mode in ("chunk", "teacher") else {}
            levels = draw_frame_levels(draw_mode, B, n_frames, device, generator, **ckw)
        noise = torch.randn(vae_latent.shape, device=device, dtype=bf16, generator=generator)
        if frame_timesteps is None:
            t, weights = frame_schedule(draw_mode, levels, n_frames, cond_prob, generator, **ckw)
        else:
            t = torch.as_tensor(frame_timesteps).to(device=device, dtype=bf16)
            weights = torch.ones(t.shape, dtype=f32, device=device)
        if frame_weights is not None:
            weights = torch.as_tensor(frame_weights).to(device=device, dtype=f32)
        if tuple(t.shape) != (B, n_frames) or tuple(weights.shape) != (B, n_frames):
            raise ValueError(f"per-frame timesteps / weights must have shape [{B}, {n_frames}] (t = T // time_patch_size), "
                             f"got {tuple(t.shape)} / {tuple(weights.shape)}")
        z_t, v_objective = ops.noise_latents_frames(vae_latent.contiguous(), noise, t.to(f32).contiguous(), pt)
        output = dit_model(z_t, caption_encoded, t, rope_start=rope_start, **kw) if rope_start is not None \
            else dit_model(z_t, caption_encoded, t, **kw)
        diffusion_loss, _per = frame_flow_loss(output, v_objective, weights, pt)
        if master_process:
            logger.debug("forward done (step %s)", global_step)
        return diffusion_loss, diffusion_loss
    z = torch.randn(B, device=device, dtype=bf16, generator=generator)
    t = time_shift_from_normal(z)
    noise = torch.randn(vae_latent.shape, device=device, dtype=bf16, generator=generator)
    z_t, v_objective = ops.noise_latents(vae_latent.contiguous(), noise, t.to(f32))
    output = dit_model(z_t, caption_encoded, t, rope_start=rope_start, **kw) if rope_start is not None \
        else dit_model(z_t, caption_encoded, t, **kw)
    diffusion_loss, _per = flow_loss(output, v_objective)
    total_loss = diffusion_loss
    if master_process:
        logger.debug("forward done (step %s)", global_step)
    return total_loss, diffusion_loss


def lr_lambda(step: int, kind: str, warmup: int, total: int) -> float:
    """multiplier of HF get_{cosine,linear}_schedule_with_warmup; "constant" is the reference's
    linear schedule with 1e10 total steps (train.py:349-364)."""
    if kind == "constant":
        kind, total = "linear", 10_000_000_000
    if step < warmup:
        return step / max(1, warmup)
    if kind == "linear":
        return max(0.0, (total - step) / max(1, total - warmup))
    if kind != "cosine":
        raise ValueError(f"unknown lr_scheduler_type {kind}")
    import math
    prog = (step - warmup) / max(1, total - warmup)
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * prog)))


def get_schedule(optimizer, lr_scheduler_type: str = "cosine", num_warmup_steps: int = 20,
                 num_training_steps: int = 10000):
    """the LR scheduler of train.py:349-364 as a torch LambdaLR (no transformers import needed)"""
    return torch.optim.lr_scheduler.LambdaLR(
        optimizer, lambda s: lr_lambda(s, lr_scheduler_type, num_warmup_steps, num_training_steps))


def train_step(dit_model, optimizer, lr_scheduler, batch, device, generator=None, rope_start=None, frame_mode=None,
               cond_prob=0.5, route=None):
    """train.py:412-434 for one batch with a pre-encoded context; returns the loss tensor.  frame_mode / cond_prob: the
    per-frame timestep modes of `forward`; route: its token-routing override."""
    fkw = {} if frame_mode is None else {"frame_mode": frame_mode, "cond_prob": cond_prob}
    if route is not None:
        fkw["route"] = route
    total_loss, _ = forward(dit_model, batch, None, None, device, 0, False, generator=generator,
                            rope_start=rope_start, **fkw)
    optimizer.zero_grad()
    total_loss.backward()
    optimizer.step()
    if lr_scheduler is not None:
        lr_scheduler.step()
    return total_loss
