"""Write tests/golden/encode16_parent.npz: what tests/test_encode16.py::record_outputs computes on the GPU with the library
of the tree this script runs in.

The committed fixture was produced by running this script in a checkout of commit c2d52e1 ("Add a ray distortion loss: HIP
kernel, autograd op, render and trainer"), the last commit whose 16-point kernels encoded their inputs per channel (one sinf
or cosf per fragment channel and lane), with only this script and tests/test_encode16.py copied in.  The test then asserts
that the current kernels give the same bits.  The forward kernels use no atomics, so the record does not vary from run to
run; `--check FILE` recomputes it and compares with an existing file instead of writing.

    python tools/gen_encode16_golden.py [--out FILE] [--check FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'encode16_parent.npz'))
    ap.add_argument('--check', default=None)
    a = ap.parse_args()
    import test_encode16
    rec = test_encode16.record_outputs(torch.device('cuda'))
    if a.check:
        want = np.load(a.check)
        assert set(want.files) == set(rec), (sorted(want.files), sorted(rec))
        bad = [k for k in rec if rec[k].tobytes() != want[k].tobytes()]
        print('arrays:', len(rec), 'differing:', bad)
        sys.exit(1 if bad else 0)
    np.savez_compressed(a.out, **rec)
    print('wrote', a.out, os.path.getsize(a.out), 'bytes;', {k: v.shape for k, v in rec.items()})


if __name__ == '__main__':
    main()
