"""Euler + classifier-free-guidance sampler on the HIP forward path (reference:
sampling/sample.py::generate_image, lines 77-159).

    acc = generate_latents(dit, prompt_embeds, inference_steps=50, cfg_scale=6.0, height=512, width=512, seed=42)

Returns the fp32 latent accumulator [1,16,16,2*(h//16),2*(w//16)] that the reference hands to the
Cosmos decoder (third-party, out of scope).  MI355X-first differences from the reference loop:
the prompt and the zeroed negative embeddings go through ONE batched forward (B=2) per step instead
of two forwards (they then share the step's random RoPE offsets -- the reference draws a second
random triple for the unconditional call), and the guidance + Euler update is one fused kernel.
`rope_starts` pins the offsets of every model call (cond, uncond per step) for parity tests; with
distinct offsets inside a step the two calls run separately, like the reference.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import ops

bf16, f32 = torch.bfloat16, torch.float32
ALPHA = 8.0  # sample.py:131


def shifted_times(i: int, steps: int) -> Tuple[float, float]:
    """(t, t_next) of step i = steps..1 after the alpha = 8 shift (sample.py:126-134)."""
    t, t_next = i / steps, (i - 1) / steps
    t = t * ALPHA / (1 + (ALPHA - 1) * t)
    t_next = t_next * ALPHA / (1 + (ALPHA - 1) * t_next)
    return t, t_next


@torch.no_grad()
def generate_latents(model, prompt_embeds: torch.Tensor, negative_embeds: Optional[torch.Tensor] = None,
                     inference_steps: int = 50, cfg_scale: float = 6.0, height: int = 512, width: int = 512,
                     seed: int = 42, latents: Optional[torch.Tensor] = None,
                     rope_starts: Optional[Sequence[Tuple[int, int, int]]] = None, device="cuda",
                     prompt_lens=None, negative_lens=None, cond_latents: Optional[torch.Tensor] = None,
                     rollout_frames: Optional[int] = None, kv_cache: bool = False) -> torch.Tensor:
    """rollout_frames = k >= 1 (frame rollout): after any cond_latents frames the remaining token-frames are generated k
    at a time, in order.  Every chunk runs the whole `inference_steps` Euler loop with per-frame timesteps -- 0 for the
    frames before the chunk, the step's t for the chunk's frames, 1.0 for the frames after it (still the initial noise)
    -- and after every Euler step the frames outside the chunk are put back, in the latents and in the accumulator, to
    the values they had when the chunk started.  Cost: (number of chunks) x inference_steps model calls (x the guided
    pair); there is no KV cache.  `rope_starts` then lists the offsets of all those calls, chunk after chunk.  Runs on
    any model; on a DiT built with frame_causal=True a finished chunk does not depend on the noise of later frames.
    None: the loop below, call for call.

    kv_cache=True (with rollout_frames, on a DiT built with frame_causal=True): the cached rollout.  Every model call
    runs on the chunk's token-frames alone (DiT.forward(frame_cache=)): the K / V rows of the finished frames come from a
    FrameKVCache and the frames after the chunk, which nothing in the chunk reads, are not computed.  One RoPE base serves
    the whole rollout (`rope_starts[0]` if given -- a list of any other length is an error -- else one draw for the full
    video), the guided pair always runs as one batched call, and the register tokens are at noise level 1.0 in every call
    (register_timesteps): a cached K / V row is only valid later if the registers were at the same level both times.
    Calls: one on any cond_latents frames at t = 0, then per chunk `inference_steps` calls on the chunk and -- after every
    chunk but the last -- one on the finished chunk at t = 0, which writes its clean K / V.  For every chunk that has
    frames after it the uncached rollout has its registers at 1.0 too (the row maximum: the frames after the chunk sit at
    1.0), so the two rollouts compute the same thing there.  On the last chunk the uncached registers follow the step's
    t, the K / V of the earlier frames then change with every step and no cache can reproduce that: the cached rollout's
    last chunk is its own defined computation -- registers at 1.0 -- pinned by tests/helpers/frame_cache_ref.py.
    False (the default): the loop described above, call for call.

    On a DiT built with frame_chunk=c > 1 (causal over chunks of c token-frames) a rollout advances by whole chunks:
    rollout_frames must be a multiple of c and the cond_latents frames a whole number of chunks (ValueError otherwise; the
    video's last chunk may be short).  kv_cache=True then takes rollout_frames == c -- a cached call covers one chunk --
    and the cond_latents prefill runs one call and one commit() per chunk.
    On a DiT built with frame_window=w the cached rollout uses the model's ring cache (new_frame_cache: w token-frames of
    K / V whatever the video's length) without further arguments; a cached call covers one chunk -- one token-frame with
    frame_chunk=1, so rollout_frames=1 there -- and the prefill runs chunk by chunk as above.  The uncached rollout runs
    the windowed full-sequence model unchanged.

    cond_latents ([1,16,Tc,h,w], Tc a multiple of the model's time_patch_size; image-to-video, video extension): the
    first Tc latent frames are held at these values -- their token-frames are given t = 0 in every model call (per-frame
    timesteps, DiT.forward), the other frames the step's t, and the frames are written back into the latents and the
    accumulator after every Euler step.  None: the loop below is the reference's.

    prompt_lens / negative_lens ([B] ints, DiT.forward's context_lens): the number of real tokens of the prompt / the
    negative prompt; if either is given every model call passes lengths, a side without them attends all its rows, and
    `negative_embeds=None` with prompt_lens means an EMPTY negative prompt (length 0: no context), not 512 zero rows.

    Samples whatever weights the model holds.  To sample the weight EMA of a training run
    (`MuAdamW(..., ema_decay=0.9999)`), either swap it in for the duration of the call

        with opt.ema_weights():
            acc = generate_latents(dit, prompt_embeds, seed=42)

    or build a sampling model from the EMA file a checkpoint carries:

        dit.load_state_dict(checkpoint.read_model_state(ckpt_dir, ema=True))
    """
    c_model = int(getattr(model, "frame_chunk", 1))
    if c_model > 1 and rollout_frames is not None and not isinstance(rollout_frames, bool) \
            and int(rollout_frames) == rollout_frames and int(rollout_frames) >= 1:  # (refused before the device is touched)
        if int(rollout_frames) % c_model != 0:
            raise ValueError(f"frame rollout on a frame_chunk={c_model} model: rollout_frames = {rollout_frames} must be a "
                             f"multiple of {c_model} -- a chunk's frames attend each other and are denoised together")
        if kv_cache and int(rollout_frames) != c_model:
            raise ValueError(f"kv_cache=True on a frame_chunk={c_model} model: a cached call covers ONE chunk, pass "
                             f"rollout_frames={c_model} (or kv_cache=False for {rollout_frames} frames at a time)")
        if cond_latents is not None and cond_latents.dim() == 5 \
                and cond_latents.shape[2] % (c_model * model.time_patch_size) != 0:
            raise ValueError(f"frame rollout on a frame_chunk={c_model} model: cond_latents must hold a whole number of "
                             f"chunks -- a multiple of {c_model * model.time_patch_size} latent frames ({c_model} token-frames "
                             f"of time_patch_size {model.time_patch_size}), got {cond_latents.shape[2]}")
    windowed = getattr(model, "frame_window", None) is not None
    if windowed and kv_cache and c_model == 1 and rollout_frames is not None and not isinstance(rollout_frames, bool) \
            and int(rollout_frames) == rollout_frames and int(rollout_frames) > 1:
        raise ValueError(f"kv_cache=True on a frame_window model with frame_chunk=1: a cached call covers ONE token-frame, "
                         f"pass rollout_frames=1 (or kv_cache=False for {rollout_frames} frames at a time)")
    dev = torch.device(device)
    prompt_embeds = prompt_embeds.to(dev, bf16)
    guided = cfg_scale > 1
    lens_c = lens_u = None
    if prompt_lens is not None or negative_lens is not None:
        from .model import check_context_lens
        nb, Lc = prompt_embeds.shape[0], prompt_embeds.shape[1]
        lens_c = check_context_lens(prompt_lens if prompt_lens is not None else [Lc] * nb, nb, Lc).to(dev)
        if guided:
            if negative_lens is None:
                negative_lens = [0] * nb if negative_embeds is None else [negative_embeds.shape[1]] * nb
            lens_u = check_context_lens(negative_lens, nb, Lc if negative_embeds is None else negative_embeds.shape[1]).to(dev)
            lens_cu = torch.cat([lens_c, lens_u])
    kw_c = {} if lens_c is None else {"context_lens": lens_c}
    kw_u = {} if lens_u is None else {"context_lens": lens_u}
    if guided and negative_embeds is None:
        negative_embeds = torch.zeros_like(prompt_embeds)  # sample.py:105
    if latents is None:
        gen = torch.Generator(device=dev).manual_seed(seed)
        latents = torch.randn((1, 16, 16, 2 * (height // 16), 2 * (width // 16)), device=dev, dtype=bf16, generator=gen)
    lat = latents.to(dev, bf16).contiguous().clone()
    acc = lat.to(f32)
    call = 0
    n_cond = 0
    k_roll = 0
    if rollout_frames is not None:
        if isinstance(rollout_frames, bool) or int(rollout_frames) != rollout_frames or int(rollout_frames) < 1:
            raise ValueError(f"rollout_frames must be an integer >= 1 (token-frames per chunk) or None, got {rollout_frames!r}")
        k_roll = int(rollout_frames)
        if lat.shape[2] % model.time_patch_size != 0:
            raise ValueError(f"frame rollout: {lat.shape[2]} latent frames are no multiple of time_patch_size "
                             f"({model.time_patch_size})")
    if kv_cache:
        if rollout_frames is None:
            raise ValueError("kv_cache=True caches the finished frames of a frame rollout: pass rollout_frames=k too")
        if not getattr(model, "frame_causal", False):
            raise ValueError("kv_cache=True needs a DiT built with frame_causal=True (without the mask the finished frames' "
                             "K / V change with the frames after them); use kv_cache=False on this model")
        if rope_starts is not None and len(rope_starts) != 1:
            raise ValueError(f"kv_cache=True: the cached rollout has ONE RoPE base, rope_starts must list exactly one "
                             f"(t, h, w), got {len(rope_starts)}")
    if cond_latents is not None:
        pt = model.time_patch_size
        Tc = cond_latents.shape[2] if cond_latents.dim() == 5 else -1
        want = (lat.shape[0], lat.shape[1], Tc, lat.shape[3], lat.shape[4])
        if Tc < 1 or Tc % pt != 0 or Tc > lat.shape[2] or tuple(cond_latents.shape) != want:
            raise ValueError(f"cond_latents must have shape [{lat.shape[0]}, {lat.shape[1]}, Tc, {lat.shape[3]}, {lat.shape[4]}] "
                             f"with Tc a multiple of time_patch_size ({pt}) and at most {lat.shape[2]}, got "
                             f"{tuple(cond_latents.shape)}")
        n_cond, n_frames = Tc // pt, lat.shape[2] // pt
        cond_acc = cond_latents.to(dev, f32)
        cond_lat = cond_acc.to(bf16)
        is_cond = torch.arange(n_frames, device=dev) < n_cond

        def impose():
            acc[:, :, :Tc] = cond_acc
            lat[:, :, :Tc] = cond_lat
        impose()

    def times(t, nb):
        """the timesteps of a model call on nb samples: [nb], or [nb, t] with the conditioning frames at 0"""
        tt = torch.tensor([t] * nb, device=dev).to(bf16)
        if not n_cond:
            return tt
        return torch.where(is_cond[None, :], torch.zeros((), dtype=bf16, device=dev), tt[:, None]).contiguous()

    def euler_loop(times, restore):
        """one pass of `inference_steps` Euler steps; times(t, nb) makes the timesteps of a model call, restore() (or
        None) runs after every step"""
        nonlocal call
        for i in range(inference_steps, 0, -1):
            t, t_next = shifted_times(i, inference_steps)
            dt = t - t_next
            if guided:
                s_c = tuple(rope_starts[call]) if rope_starts is not None else None
                s_u = tuple(rope_starts[call + 1]) if rope_starts is not None else None
                call += 2
                if s_c == s_u:  # one batched forward: [cond, uncond]
                    tt = times(t, 2)
                    out = model(torch.cat([lat, lat]), torch.cat([prompt_embeds, negative_embeds.to(dev, bf16)]), tt,
                                **({"rope_start": s_c} if s_c is not None else {}),
                                **({} if lens_c is None else {"context_lens": lens_cu}))
                    cond, uncond = out[0:1].contiguous(), out[1:2].contiguous()
                else:
                    tt = times(t, 1)
                    cond = model(lat, prompt_embeds, tt, rope_start=s_c, **kw_c)
                    uncond = model(lat, negative_embeds.to(dev, bf16), tt, rope_start=s_u, **kw_u)
            else:
                tt = times(t, 1)
                s_c = tuple(rope_starts[call]) if rope_starts is not None else None
                call += 1
                cond = model(lat, prompt_embeds, tt, **({"rope_start": s_c} if s_c is not None else {}), **kw_c)
                uncond = None
            ops.cfg_euler_step(cond, uncond, acc, lat, cfg_scale, dt)
            if restore is not None:
                restore()

    if rollout_frames is None:
        euler_loop(times, impose if n_cond else None)
        return acc

    # frame rollout: chunk after chunk of k token-frames, each with its own full Euler pass
    pt = model.time_patch_size
    n_frames = lat.shape[2] // pt
    if kv_cache:
        p = model.patch_size
        nb = 2 if guided else 1
        base = tuple(rope_starts[0]) if rope_starts is not None else model.rope.draw_start(
            (n_frames, lat.shape[3] // p, lat.shape[4] // p))
        cache = model.new_frame_cache(nb, n_frames, lat.shape[3] // p, lat.shape[4] // p, device=dev)
        ctx = torch.cat([prompt_embeds, negative_embeds.to(dev, bf16)]) if guided else prompt_embeds
        kw = {} if lens_c is None else {"context_lens": lens_cu if guided else lens_c}
        reg = torch.ones(nb, dtype=f32, device=dev)

        def chunk_call(f0, f1, t):
            """the model on token-frames f0 .. f1 at noise level t, the frames before them read from the cache"""
            x = lat[:, :, f0 * pt:f1 * pt]
            tt = torch.full((nb, f1 - f0), float(t), device=dev).to(bf16)
            return model(torch.cat([x, x]) if guided else x.contiguous(), ctx, tt,
                         rope_start=(base[0] + f0, base[1], base[2]), register_timesteps=reg, frame_cache=cache, **kw)

        # (frame_chunk, or a ring cache: one call and one commit per chunk)
        per_chunk = c_model > 1 or windowed
        for f0 in range(0, n_cond, c_model if per_chunk else max(n_cond, 1)):
            chunk_call(f0, min(f0 + c_model, n_cond) if per_chunk else n_cond, 0.0)
            cache.commit()
        for f0 in range(n_cond, n_frames, k_roll):
            f1 = min(f0 + k_roll, n_frames)
            lat_c = lat[:, :, f0 * pt:f1 * pt].contiguous()
            acc_c = acc[:, :, f0 * pt:f1 * pt].contiguous()
            for i in range(inference_steps, 0, -1):
                t, t_next = shifted_times(i, inference_steps)
                out = chunk_call(f0, f1, t)
                cond, uncond = (out[0:1].contiguous(), out[1:2].contiguous()) if guided else (out, None)
                ops.cfg_euler_step(cond, uncond, acc_c, lat_c, cfg_scale, t - t_next)
                lat[:, :, f0 * pt:f1 * pt] = lat_c
                acc[:, :, f0 * pt:f1 * pt] = acc_c
            if f1 < n_frames:
                chunk_call(f0, f1, 0.0)  # the finished chunk's clean K / V
                cache.commit()
        return acc
    frame = torch.arange(n_frames, device=dev)
    for f0 in range(n_cond, n_frames, k_roll):
        f1 = min(f0 + k_roll, n_frames)
        acc0, lat0 = acc.clone(), lat.clone()  # the finished frames before the chunk, the initial noise after it

        def chunk_times(t, nb, f0=f0, f1=f1):
            row = torch.where(frame < f0, 0.0, torch.where(frame < f1, float(t), 1.0)).to(bf16)
            return row[None, :].expand(nb, n_frames).contiguous()

        def restore(f0=f0, f1=f1, acc0=acc0, lat0=lat0):
            for cur, old in ((acc, acc0), (lat, lat0)):
                cur[:, :, :f0 * pt] = old[:, :, :f0 * pt]
                cur[:, :, f1 * pt:] = old[:, :, f1 * pt:]
        euler_loop(chunk_times, restore)
    return acc
