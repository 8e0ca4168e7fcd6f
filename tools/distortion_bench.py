"""Time of the distortion-loss kernel (csrc/distortion.hip) at frame size -- 378 x 504 rays, S = 128 and S = 192, loss only and
loss + gradient -- against a fp32 torch composition of the same recurrences (cumsum-based, forward + autograd backward).

  python tools/distortion_bench.py                     the launches, in the fixed order of CONFIGS (LAUNCHES each), for
        `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python3 tools/distortion_bench.py`; also times
        both with device events in this process and writes $MVIP_PROFILE_OUT/distortion_bench.json (default: profile_out/)
  python tools/distortion_bench.py --trace DIR/.../run_kernel_trace.csv
        no GPU: cuts the kernel's dispatches out of that trace, LAUNCHES per config in order, and merges min / mean and the share
        of the 6.3 TB/s copy rate into the JSON written by the run
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RAYS = 378 * 504
LAUNCHES = 20
COPY_RATE = 6.3e12                                       # B/s, the copy rate the HBM-bound kernels here are read against
# (samples per ray, gradient asked for, lindisp)
CONFIGS = [(128, False, False), (128, True, False), (192, False, False), (192, True, False), (128, False, True), (128, True, True)]


def algorithmic_bytes(S, grad):
    return RAYS * (S * 8 + 8 + 4 + (S * 4 if grad else 0))       # z + weights, near / far, loss, and the gradient row


def name(S, grad, lindisp):
    return f'S{S}_{"loss_grad" if grad else "loss_only"}{"_lindisp" if lindisp else ""}'


def torch_composition(w, z, near, far):
    """The recurrences of csrc/distortion.hip as stock fp32 torch ops (plain normalisation)."""
    import torch
    s = (z - near) / (far - near)
    m = torch.cat([0.5 * (s[:, :-1] + s[:, 1:]), s[:, -1:]], 1)
    d = torch.cat([s[:, 1:] - s[:, :-1], torch.zeros_like(s[:, :1])], 1)
    W_lt = torch.cumsum(w, 1) - w
    dm = torch.cat([torch.zeros_like(m[:, :1]), m[:, 1:] - m[:, :-1]], 1)
    D = torch.cumsum(dm * W_lt, 1)
    return (w * (2.0 * D + w * d / 3.0)).sum(1)


def run_gpu(out_path):
    import torch
    from mvip_nerf_amd import ops
    from tools.render_occupancy_ab import event_ms
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    rows = torch.zeros((RAYS, 11), device=dev)
    rows[:, 6], rows[:, 7] = 1.2, 7.74
    out = {'rays': RAYS, 'launches_per_config': LAUNCHES, 'order': [name(*c) for c in CONFIGS], 'device_events': {}, 'torch_composition': {}}
    for S, grad, lindisp in CONFIGS:
        z = torch.sort(1.2 + 6.54 * torch.rand((RAYS, S), device=dev), 1)[0].contiguous()
        w = (torch.rand((RAYS, S), device=dev) / S).requires_grad_(grad)
        ms = [event_ms(lambda: ops.distortion_loss(w, z, rows, lindisp)) for _ in range(LAUNCHES)]
        out['device_events'][name(S, grad, lindisp)] = {'ms_min': min(ms), 'ms_mean': sum(ms) / len(ms), 'bytes': algorithmic_bytes(S, grad)}
        if grad and not lindisp:                        # the composition: forward + backward, the kernel: forward (which holds
            def both():                                 # the gradient) + the backward's elementwise product
                loss = ops.distortion_loss(w, z, rows, lindisp)
                return torch.autograd.grad(loss.sum(), w)[0]

            def stock():
                return torch.autograd.grad(torch_composition(w, z, 1.2, 7.74).sum(), w)[0]
            a, b = both(), stock()
            k_ms, t_ms = [], []
            for _ in range(5):
                k_ms.append(event_ms(both))
                t_ms.append(event_ms(stock))
            out['torch_composition'][f'S{S}'] = {
                'kernel_forward_backward_ms': k_ms, 'torch_forward_backward_ms': t_ms, 'speedup_of_minima': min(t_ms) / min(k_ms),
                'max_abs_gradient_difference': float((a - b).abs().max()), 'max_abs_gradient': float(a.abs().max())}
    torch.cuda.synchronize()
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(out, open(out_path, 'w'), indent=1)


def merge_trace(trace, out_path):
    rows = [r for r in csv.DictReader(open(trace)) if 'distortion_loss_kernel' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    us = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows]
    # per config: LAUNCHES timed launches; the S x gradient configs that feed the composition comparison add 1 + 5 more, skipped here
    out = json.load(open(out_path)) if os.path.exists(out_path) else {}
    out['kernel_trace'], at = {}, 0
    for S, grad, lindisp in CONFIGS:
        t = us[at:at + LAUNCHES]
        at += LAUNCHES + (6 if grad and not lindisp else 0)
        assert len(t) == LAUNCHES, f'{len(us)} dispatches in the trace: not the launch order of this tool'
        b = algorithmic_bytes(S, grad)
        out['kernel_trace'][name(S, grad, lindisp)] = {
            'us_min': min(t), 'us_mean': sum(t) / len(t), 'bytes': b, 'share_of_copy_rate_at_min': b / (min(t) * 1e-6) / COPY_RATE,
            'share_of_copy_rate_at_mean': b / (sum(t) / len(t) * 1e-6) / COPY_RATE}
    assert at == len(us), f'{len(us)} dispatches in the trace, {at} expected'
    print(json.dumps(out['kernel_trace'], indent=1))
    json.dump(out, open(out_path, 'w'), indent=1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--trace', default=None)
    a = ap.parse_args(argv)
    out_path = os.path.join(os.environ.get('MVIP_PROFILE_OUT', 'profile_out'), 'distortion_bench.json')
    if a.trace:
        merge_trace(a.trace, out_path)
    else:
        run_gpu(out_path)
    return 0


if __name__ == '__main__':
    sys.exit(main())
