"""Host-side checks of the 2D sampler (guidance/sd_utils.StableDiffusion.produce_latents / inpaint / prompt_to_img): the DDIM
schedule and one update against an fp64 restatement of the equations, strength validation, and the public signatures
against the reference's (DS_NeRF/guidance/sd_utils.py:111, :602-666)."""
import inspect
import math

import numpy as np
import pytest
import torch

from mvip_nerf_amd.guidance import sd_utils
from mvip_nerf_amd.guidance.sd_nets import scaled_linear_alphas_cumprod


def _alphas64():
    b = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    return np.cumprod(1.0 - b)


@pytest.mark.parametrize('n', [1, 4, 7, 50, 1000])
def test_ddim_timesteps_sd1x_leading_offset_one(n):
    ts, ratio = sd_utils.ddim_timesteps(n)
    assert ratio == 1000 // n
    assert ts == [int(v) for v in (np.arange(n) * (1000 // n))[::-1] + 1]
    assert len(ts) == n and ts[-1] == 1
    if n == 50:
        assert ts[:3] == [981, 961, 941]


@pytest.mark.parametrize('n,strength,count', [(50, 1.0, 50), (50, 0.5, 25), (50, 0.33, 16), (4, 0.5, 2), (10, 0.05, 0)])
def test_get_timesteps(n, strength, count):
    ts, _ = sd_utils.ddim_timesteps(n)
    got, m = sd_utils.get_timesteps(ts, n, strength)
    init = min(int(n * strength), n)                  # pipeline_sd_inpainting.py:751-758
    t_start = max(n - init, 0)
    assert m == n - t_start == count
    assert got == ts[t_start:]


def test_ddim_update_matches_fp64_equations():
    """One update from ddim_step_scalars' block, evaluated as the kernel evaluates it (fp32) and in fp64 from the
    equations: e = e_u + g (e_c - e_u); x0 = (x - sqrt(1 - a_t) e) / sqrt(a_t); x' = sqrt(a_p) x0 + sqrt(1 - a_p) e."""
    alphas_host = [float(a) for a in scaled_linear_alphas_cumprod()]
    a64 = _alphas64()
    np.testing.assert_allclose(alphas_host, a64, rtol=2e-6)
    rng = np.random.default_rng(0)
    eu, ec, x = (rng.standard_normal(4 * 64 * 64) for _ in range(3))
    for t, ratio, g in ((981, 20, 7.5), (21, 20, 7.5), (1, 20, 3.0), (501, 250, 1.0)):
        scal = sd_utils.ddim_step_scalars(alphas_host, t, ratio, g, t_next=t - ratio)
        assert len(scal) == 6 and scal[0] == g and scal[5] == float(t - ratio)
        at = a64[t]
        ap = a64[t - ratio] if t - ratio >= 0 else a64[0]          # set_alpha_to_one = False
        e = eu + g * (ec - eu)
        ref = math.sqrt(ap) * (x - math.sqrt(1 - at) * e) / math.sqrt(at) + math.sqrt(1 - ap) * e
        s = np.asarray(scal, np.float32)
        e32 = (eu.astype(np.float32) + s[0] * (ec.astype(np.float32) - eu.astype(np.float32))).astype(np.float32)
        x0 = ((x.astype(np.float32) - s[2] * e32) / s[1]).astype(np.float32)
        got = (s[3] * x0 + s[4] * e32).astype(np.float32)
        # fp32 evaluation against fp64 (the table itself is fp32: 9.3e-7 relative): measured worst 2.3e-6 of max |ref|
        # (t = 21); bound 2e-5 (~8x headroom)
        assert float(np.abs(got - ref).max() / np.abs(ref).max()) < 2e-5, (t, ratio)


@pytest.mark.parametrize('bad', [0, 0.0, -0.1, 1.0001, 2, float('nan'), '0.5', None])
def test_strength_outside_open_closed_unit_interval_raises(bad):
    with pytest.raises(ValueError):
        sd_utils._check_strength(bad)


@pytest.mark.parametrize('ok', [1, 1.0, 0.5, 1e-3])
def test_strength_inside_accepted(ok):
    sd_utils._check_strength(ok)


# the reference's signatures (DS_NeRF/guidance/sd_utils.py:111, :602, :624, :633, :643), hard-coded
REFERENCE = {
    'get_text_embeds': [('prompt', inspect.Parameter.empty)],
    'produce_latents': [('text_embeddings', inspect.Parameter.empty), ('height', 512), ('width', 512),
                        ('num_inference_steps', 50), ('guidance_scale', 7.5), ('latents', None)],
    'decode_latents': [('latents', inspect.Parameter.empty)],
    'encode_imgs': [('imgs', inspect.Parameter.empty)],
    'prompt_to_img': [('prompts', inspect.Parameter.empty), ('negative_prompts', ''), ('height', 512), ('width', 512),
                      ('num_inference_steps', 50), ('guidance_scale', 7.5), ('latents', None)],
}
EXTRAS = {'produce_latents': [('mask', None), ('masked_image_latents', None)]}


@pytest.mark.parametrize('name', sorted(REFERENCE))
def test_signatures_equal_the_reference_plus_keyword_only_extras(name):
    ps = list(inspect.signature(getattr(sd_utils.StableDiffusion, name)).parameters.values())
    assert ps[0].name == 'self'
    pos = [(p.name, p.default) for p in ps[1:] if p.kind == p.POSITIONAL_OR_KEYWORD]
    kw = [(p.name, p.default) for p in ps[1:] if p.kind == p.KEYWORD_ONLY]
    assert pos == REFERENCE[name]
    assert kw == EXTRAS.get(name, [])
    assert len(ps) == 1 + len(pos) + len(kw)


def test_inpaint_signature():
    ps = inspect.signature(sd_utils.StableDiffusion.inpaint).parameters
    assert [(p.name, p.default) for p in list(ps.values())[1:]] == [
        ('image', inspect.Parameter.empty), ('mask', inspect.Parameter.empty), ('prompt', inspect.Parameter.empty),
        ('negative_prompt', ''), ('num_inference_steps', 50), ('guidance_scale', 7.5), ('strength', 1.0), ('latents', None)]


def test_inpaint_rejects_bad_strength_before_any_work():
    sd = sd_utils.StableDiffusion.__new__(sd_utils.StableDiffusion)      # no networks: validation comes first
    for bad in (0.0, 1.5, -1):
        with pytest.raises(ValueError):
            sd.inpaint(torch.zeros(1, 3, 8, 8), torch.zeros(1, 1, 8, 8), 'x', strength=bad)


def test_sampler_sizes_other_than_512_not_implemented():
    with pytest.raises(NotImplementedError):
        sd_utils.StableDiffusion._check_size(256, 512)
    sd_utils.StableDiffusion._check_size(512, 512)


def test_decoder_image_host_path_is_the_torch_expression():
    """Decoder.image on host tensors = clamp(forward / 2 + 0.5, 0, 1) and rint(255 .) (the CPU reference of the head kernel)."""
    from mvip_nerf_amd.guidance.sd_nets import Decoder
    torch.manual_seed(0)
    dec = Decoder(block_out=(32, 32, 32, 32)).eval()
    z = torch.randn(1, 4, 4, 4)
    with torch.no_grad():
        img, u8 = dec.image(z, uint8=True)
        ref = (dec(z) / 2 + 0.5).clamp(0, 1)
    assert img.shape == (1, 3, 32, 32) and u8.shape == (1, 32, 32, 3) and u8.dtype == torch.uint8
    torch.testing.assert_close(img, ref, rtol=0, atol=0)
    torch.testing.assert_close(u8, (ref * 255).round().to(torch.uint8).permute(0, 2, 3, 1), rtol=0, atol=0)
