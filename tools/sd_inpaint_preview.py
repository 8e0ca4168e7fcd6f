"""2D inpainting preview of the SDS prior: what StableDiffusion.inpaint paints into a rectangle of a training view for a prompt,
in seconds instead of thousands of SDS iterations.  Writes a PNG and prints the decode time, the per-step time and the decoder
head kernel's share of HBM bandwidth (these are the figures DESIGN.md and profiles/sd_sampler.json record).

  python tools/sd_inpaint_preview.py [--scene NPZ --view K: a tests/golden scene view by default] [--rect y0 x0 y1 x1]
      [--prompt TEXT] [--hf_key DIR] [--steps N] [--out DIR] [--json FILE]

Without --hf_key the networks hold seeded random weights: the image is noise-like, the timings are those of the real shapes."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # MI355X HBM3E, bytes / s (spec)


def _events_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--scene', default=os.path.join(ROOT, 'tests', 'golden', 'scene1_f8.npz'))
    ap.add_argument('--view', type=int, default=0)
    ap.add_argument('--rect', type=int, nargs=4, default=None, help='mask rectangle y0 x0 y1 x1 (default: the centre quarter)')
    ap.add_argument('--prompt', default='a stone bench in a park')
    ap.add_argument('--hf_key', default=None, help='diffusers-layout checkpoint DIRECTORY (random weights without)')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--guidance', type=float, default=7.5)
    ap.add_argument('--strength', type=float, default=1.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--fp16', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profile_out'))
    ap.add_argument('--json', default=None, help='also write the figures to this JSON file')
    a = ap.parse_args(argv)

    import torch
    from mvip_nerf_amd import ops
    from mvip_nerf_amd.run import _write_png
    from mvip_nerf_amd.guidance.sd_utils import StableDiffusion
    if not torch.cuda.is_available():
        raise SystemExit('needs the GPU (the sampler runs on the HIP kernels only)')
    dev = torch.device('cuda', 0)
    rgb = np.load(a.scene)['images'][a.view]
    H, W = rgb.shape[:2]
    y0, x0, y1, x1 = a.rect or (H // 4, W // 4, 3 * H // 4, 3 * W // 4)
    image = torch.from_numpy(rgb).to(dev).permute(2, 0, 1)[None].float() / 255.0
    mask = torch.zeros(1, 1, H, W, device=dev)
    mask[:, :, y0:y1, x0:x1] = 1

    torch.manual_seed(a.seed)
    sd = StableDiffusion(dev, a.fp16, False, hf_key=a.hf_key)
    sd.seed_generator(a.seed)
    sd.inpaint(image, mask, a.prompt, num_inference_steps=2, guidance_scale=a.guidance)       # capture + warm-up
    torch.cuda.synchronize()
    sd.seed_generator(a.seed)
    t0 = time.perf_counter()
    img = sd.inpaint(image, mask, a.prompt, num_inference_steps=a.steps, guidance_scale=a.guidance, strength=a.strength)
    torch.cuda.synchronize()
    total_ms = (time.perf_counter() - t0) * 1e3

    # per-step time: replays of the captured step alone (n steps minus 1 step, same call otherwise)
    lat = torch.randn(1, 4, 64, 64, device=dev, generator=sd.generator)
    emb = sd.networks.encode_prompt(a.prompt, a.guidance > 1.0)
    kw = dict(num_inference_steps=a.steps, guidance_scale=a.guidance, latents=lat)
    t_n = _events_ms(lambda: sd.produce_latents(emb, **kw), 3)
    kw['num_inference_steps'] = 1
    t_1 = _events_ms(lambda: sd.produce_latents(emb, **kw), 3)
    step_ms = (t_n - t_1) / max(a.steps - 1, 1)
    decode_ms = _events_ms(lambda: sd.decode_latents(lat), 5)

    # the head kernel alone, at the decoder's last level (128 channels at 512 x 512): bytes it must move / its time
    dec = sd.vae.decoder
    x = torch.randn(1, dec.conv_norm_out.num_channels, 512, 512, device=dev)
    with ops.precision(sd.vae.mfma_prec):
        head_ms = _events_ms(lambda: ops.vae_decoder_head(x, dec.conv_norm_out, dec.conv_out, uint8=True), 20)
        ws = ops._gn_workspace(1, x.shape[1], 512 * 512, dev)
        stats_ms = _events_ms(lambda: ops._gn_stats(x, 1, x.shape[1], 512, 512, 32, 1e-6, ws), 20)
    kernel_ms = head_ms - stats_ms
    head_bytes = x.numel() * 4 + 512 * 512 * 3 * (4 + 1)
    head_frac = head_bytes / (kernel_ms * 1e-3) / HBM_PEAK

    os.makedirs(a.out, exist_ok=True)
    png = os.path.join(a.out, 'sd_inpaint_preview.png')
    _write_png(png, (img[0].permute(1, 2, 0).clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy())
    res = {'steps': a.steps, 'inpaint_ms': round(total_ms, 2), 'step_ms': round(step_ms, 3), 'decode_ms': round(decode_ms, 3),
           'head_ms_with_stats': round(head_ms, 4), 'groupnorm_stats_ms': round(stats_ms, 4), 'head_kernel_ms': round(kernel_ms, 4),
           'head_kernel_bytes': head_bytes, 'head_kernel_GBps': round(head_bytes / (kernel_ms * 1e-3) / 1e9, 1),
           'head_kernel_hbm_fraction': round(head_frac, 3), 'weights': 'checkpoint' if a.hf_key else 'seeded random',
           'fp16': a.fp16, 'png': os.path.relpath(png, ROOT)}
    print(json.dumps(res))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == '__main__':
    main()
