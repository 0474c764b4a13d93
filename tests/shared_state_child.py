"""Child process of tests/test_gpu_shared_state.py (started with subprocess: its assertions need a runtime nobody has used yet --
no ticket pool, no tail-split scratch -- which no test inside a long pytest process can have).  Prints ONE JSON line of
observations; the parent asserts on them.  Sequence:

  1. before anything ran, and after an eager launch of the PLAIN schedule (par_split = 0): every field of sg_runtime_state is 0;
  2. the first launch that ASKS for scratch is a capture: the captured scratch is still empty, sg_tail_scratch returns nullptr, the
     capture takes the plain schedule and draws no counter;
  3. eager warm-up of the parity-split transposed conv, capture as graph A;
  4. the F(4x4,3x3) half-round conv eagerly: it asks for more scratch than the parity split did, so the scratch of the stream and
     the scratch shared by captures are both REPLACED (graph A keeps the address of the old one); capture as graph B;
  5. replays A, B, A, B against the eager results; the counters afterwards.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    from scene_generation_amd import ops, _hip
    dev = 'cuda'
    obs = {}
    g = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda *shape: torch.rand(*shape, device=dev, generator=g) * 2 - 1
    px, pw, pb = rnd(2, 512, 8, 8), rnd(512, 256, 3, 3) * 0.05, rnd(256) * 0.2
    fx, fw, fb = rnd(32, 1024, 8, 8), rnd(1024, 1024, 3, 3) * 0.05, rnd(1024) * 0.2
    par = lambda: ops.conv_transpose2d(px, pw, pb, stride=2, pad=1, out_pad=1)
    f43 = lambda: ops.conv2d(fx, fw, fb, pad=1, reflect=True)
    torch.cuda.synchronize()
    obs['fresh'] = ops.runtime_state(True)
    with torch.no_grad():
        _hip.set_option('par_split', 0)
        y_plain = par().clone()                          # (also builds the shape tables: a capture cannot)
        _hip.set_option('par_split', 1)
        obs['after_plain'] = ops.runtime_state(True)
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0):
            y0 = par()
        obs['after_cold_capture'] = ops.runtime_state()
        g0.replay()
        obs['cold_capture_equals_plain'] = bool(torch.equal(y0, y_plain))
        y_par = par().clone()                            # eager: creates the ring, the scratch and the captured scratch
        obs['par_split_differs_from_plain'] = not bool(torch.equal(y_par, y_plain))
        obs['after_par_eager'] = ops.runtime_state()
        ga = torch.cuda.CUDAGraph()
        with torch.cuda.graph(ga):
            ya = par()
        obs['after_capture_a'] = ops.runtime_state()
        y_f43 = f43().clone()
        obs['after_f43_eager'] = ops.runtime_state()
        gb = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gb):
            yb = f43()
        obs['after_capture_b'] = ops.runtime_state()
        same = []
        for _ in range(2):
            ga.replay()
            same.append(bool(torch.equal(ya, y_par)))
            gb.replay()
            same.append(bool(torch.equal(yb, y_f43)))
        obs['replays_equal_eager'] = same
        obs['after_replays'] = ops.runtime_state(True)
    print(json.dumps(obs))


if __name__ == '__main__':
    main()
