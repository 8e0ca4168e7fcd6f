"""feature_linear folded into the view layer (NeRF.fold_feature_inference, csrc/mlp_fwd16_fold.hip) against the unfolded
launches, in ONE process, settings alternated, device events:
  (a) the fine-pass network launch at the bench shape (190,512 rays x 128 samples),
  (b) the fused coarse launch on one 32,768-ray chunk, (b2) the fused fine launch on the same chunk,
  (c) whole frames as bench.py's step() renders them,
  (d) one fold pack against one mvip_mlp_pack16 + mvip_mlp_pack of the same weights,
  (e) max |delta| of rgb_map / depth_map / acc_map between the two settings on the bench frame.
Prints one JSON and writes it to $MVIP_PROFILE_OUT/fold_feature_ab.json (default folder: profile_out/).  `--launch-only` runs (a) alone (for a counter pass)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                   # noqa: E402
from mvip_nerf_amd import run, ops                             # noqa: E402

REPEATS = 3
FLOP_REFERENCE = 2 * 593408          # per point, the reference network (what bench.py --full counts)
FLOP_FOLDED = 2 * 527872             # per point, executed with the fold (the 256 x 256 feature layer gone)
PEAK_F32_TFLOPS = 157.3


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    tr, te, *_ = run.create_nerf(bench.make_args(), device=dev)
    nets = (te['network_fn'], te['network_fine'])
    H, W, F, NEAR, FAR = bench.H, bench.W, bench.FOCAL, bench.NEAR, bench.FAR
    rows = ops.ray_rows_from_pose(bench.orbit_pose(0, dev), H, W, F, NEAR, FAR)
    z128 = ops.stratified_z(rows, 128, True)
    chunk = rows[:1 << 15].contiguous()
    zc = z128[:1 << 15].contiguous()
    u = torch.linspace(0., 1., 64, device=dev)
    fine = te['network_fine']
    ps, packed = fine.param_list(), fine.packed()

    def set_fold(on):
        for n in nets:
            n.fold_feature_inference = on

    def frame(k=1):
        return run.render(H, W, F, chunk=1 << 15, c2w=bench.orbit_pose(k, dev), near=NEAR, far=FAR, **te)

    out = {'shape': {'fine_launch_points': int(rows.shape[0]) * 128, 'chunk_rays': 1 << 15, 'frame': [H, W]},
           'fine_launch_ms': {'unfolded': [], 'folded': []}, 'coarse_fused_chunk_ms': {'unfolded': [], 'folded': []},
           'fine_fused_chunk_ms': {'unfolded': [], 'folded': []}, 'frame_ms': {'unfolded': [], 'folded': []}}
    launch_only = '--launch-only' in sys.argv
    with torch.no_grad():
        for rep in range(REPEATS):
            for name, on in (('unfolded', False), ('folded', True)):
                set_fold(on)
                img = fine.packed_w16()
                out['fine_launch_ms'][name].append(event_ms(lambda: ops.mlp_rays(rows, z128, packed, ps, packed16=img), 3))
                if launch_only:
                    continue
                out['coarse_fused_chunk_ms'][name].append(
                    event_ms(lambda: ops.render_coarse_fused(img, chunk, True, None, None, u, True), 5))
                out['fine_fused_chunk_ms'][name].append(event_ms(lambda: ops.render_fine_fused(img, chunk, zc, None, True), 5))
                out['frame_ms'][name].append(event_ms(frame, 3))
        pts = int(rows.shape[0]) * 128
        best = {k: min(v) for k, v in out['fine_launch_ms'].items()}
        out['fine_launch_tflops'] = {
            'unfolded_executed': pts * FLOP_REFERENCE / best['unfolded'] / 1e9,
            'folded_executed': pts * FLOP_FOLDED / best['folded'] / 1e9,
            'folded_reference_work': pts * FLOP_REFERENCE / best['folded'] / 1e9}
        out['fine_launch_frac_of_peak'] = {k: v / PEAK_F32_TFLOPS for k, v in out['fine_launch_tflops'].items()}
        if not launch_only:
            # (d) one fold pack / one repack of the existing images
            ext = ops.mlp_pack16(ps, packed, fold=False)
            out['pack_ms'] = {'fold_pack16': event_ms(lambda: ops.mlp_fold_pack16(ps, ext), 20),
                              'pack16_plain': event_ms(lambda: ops.mlp_pack16(ps, packed, fold=False), 20),
                              'pack32': event_ms(lambda: ops.mlp_pack(ps), 20)}
            # (e) how far the maps move
            maps = {}
            for name, on in (('unfolded', False), ('folded', True)):
                set_fold(on)
                r = frame()
                maps[name] = dict(rgb_map=r[0], acc_map=r[2], depth_map=r[3])          # render(): [rgb, disp, acc, depth, extras]
            out['max_abs_delta'] = {k: float((maps['folded'][k] - maps['unfolded'][k]).abs().max()) for k in maps['folded']}
    set_fold(True)
    print(json.dumps(out, indent=1))
    out_dir = os.environ.get('MVIP_PROFILE_OUT', 'profile_out')
    os.makedirs(out_dir, exist_ok=True)
    json.dump(out, open(os.path.join(out_dir, 'fold_feature_ab' + ('_launch_only' if launch_only else '') + '.json'), 'w'), indent=1)


if __name__ == '__main__':
    main()
