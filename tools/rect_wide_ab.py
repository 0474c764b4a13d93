"""A/B of conv2d_rect / conv2d_wide between two builds of the library: are the outputs bit-equal and the reported plans equal?

  python tools/rect_wide_ab.py --a <libA.so> --b <libB.so> --report <file>     (build a side library with tools/build_variant.sh)

Each library runs in a fresh child process of its own (SG_LIB_PATH), never both in one: the child calls the two operators on seeded
inputs -- rows of tests/test_gpu_inception.py / tests/test_gpu_lpips.py, one per tile class and weight-load form, the split-K rows,
and a wide split-K shape -- into a channel slice with bias + ReLU and plain, with aligned and with offset weights, and saves every
output and every reported plan to an .npz.  The parent compares the two files on the host and writes the report."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#        name                         N  C     Cout H    W    KH  KW  s  pH pW
CASES = {'rect': [('1x7_every_row_pads', 2, 5, 7, 9, 6, 1, 7, 1, 0, 3),
                  ('7x1_on_9x6', 2, 5, 7, 9, 6, 7, 1, 1, 3, 0),
                  ('1x7_128_on_17', 2, 128, 128, 17, 17, 1, 7, 1, 0, 3),
                  ('7x1_128_on_17', 2, 128, 128, 17, 17, 7, 1, 1, 3, 0),
                  ('k3s2_288to384_on_35', 1, 288, 384, 35, 35, 3, 3, 2, 0, 0),
                  ('k5p2_48to64_on_35', 2, 48, 64, 35, 35, 5, 5, 1, 2, 2),
                  ('k3p1_K27', 2, 3, 32, 10, 7, 3, 3, 1, 1, 1),
                  ('k3_32to32_vector_weights', 2, 32, 32, 9, 11, 3, 3, 1, 0, 0),
                  ('k1_2048to192_split', 1, 2048, 192, 8, 8, 1, 1, 1, 0, 0),
                  ('k1_4to64_on_224_wide_tile', 2, 4, 64, 224, 224, 1, 1, 1, 0, 0)],
         'wide': [('alex_stem_64', 1, 3, 64, 64, 64, 11, 11, 4, 2, 2),
                  ('alex_stem_rect', 2, 3, 64, 43, 30, 11, 11, 4, 2, 2),
                  ('k7s3', 2, 5, 33, 16, 13, 7, 7, 3, 3, 3),
                  ('k11x3_vec', 2, 4, 65, 29, 9, 11, 3, 4, 0, 1),
                  ('k3p1_256to384_on_13_split', 1, 256, 384, 13, 13, 3, 3, 1, 1, 1)]}
EXTRA = 3                   # channels of the result outside the slice (2 before, 1 after)


def child(out_path):
    import torch
    sys.path.insert(0, ROOT)
    from scene_generation_amd import ops
    dev = torch.device('cuda:0')
    saved = {}
    for family, conv, query in (('rect', ops.conv2d_rect, ops.conv2d_rect_plan), ('wide', ops.conv2d_wide, ops.conv2d_wide_plan)):
        for name, n, c, cout, h, w, kh, kw, s, ph, pw in CASES[family]:
            g = torch.Generator().manual_seed(n + c + cout + h + w + 7 * kh + kw)
            x = torch.randn(n, c, h, w, generator=g).to(dev)
            wt = (torch.randn(cout, c, kh, kw, generator=g) * (2.0 / (c * kh * kw)) ** 0.5).to(dev)
            b = (0.3 * torch.randn(cout, generator=g)).to(dev)
            pad1 = torch.empty(wt.numel() + 4, device=dev)
            w_off = pad1[1:1 + wt.numel()].view_as(wt).copy_(wt)            # 4 bytes past a 16-byte boundary: scalar weight loads
            d = ops.rect_desc(n, c, h, w, cout, kh, kw, s, ph, pw, 2, cout + EXTRA)
            for wname, wv in (('aligned', wt), ('offset', w_off)):
                key = '%s/%s/%s' % (family, name, wname)
                saved[key + '/plan'] = np.frombuffer(json.dumps(query(d, wv.data_ptr() % 16 == 0), sort_keys=True).encode(), dtype=np.uint8)
                for variant, bias, act in (('bias_relu', b, ops.ACT_RELU), ('plain', None, ops.ACT_NONE)):
                    out = torch.full((n, cout + EXTRA, d.OH, d.OW), -12345.0, device=dev)
                    conv(x, wv, bias, stride=s, pad=(ph, pw), act=act, out=out, out_c0=2)
                    saved['%s/%s' % (key, variant)] = out.cpu().numpy()
    torch.cuda.synchronize()
    np.savez(out_path, **saved)


def compare(path_a, path_b, report, names):
    a, b = np.load(path_a), np.load(path_b)
    lines = ['conv2d_rect / conv2d_wide, A = %s, B = %s' % names, 'each output: [N, Cout + %d, OH, OW] float32, compared as bytes' % EXTRA, '']
    ok = sorted(a.files) == sorted(b.files)
    for key in sorted(k for k in a.files if k.endswith('/plan')):
        pa, pb = a[key].tobytes().decode(), b[key].tobytes().decode()
        outs = [k for k in a.files if k.startswith(key[:-4]) and not k.endswith('/plan')]
        eq = all(k in b.files and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in outs)
        ok = ok and eq and pa == pb
        lines.append('%-52s shape %-20s plan A %s' % (key[:-5], 'x'.join(str(v) for v in a[outs[0]].shape), pa))
        lines.append('%-52s %d outputs bit-equal: %s   plan equal: %s' % ('', len(outs), 'yes' if eq else 'NO', 'yes' if pa == pb else 'NO, B %s' % pb))
    lines += ['', 'bit-equal: %s' % ('yes' if ok else 'no')]
    text = '\n'.join(lines) + '\n'
    print(text)
    if report:
        with open(report, 'w') as f:
            f.write(text)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--a', help='library A (default: the built one)')
    ap.add_argument('--b', help='library B')
    ap.add_argument('--names', default='A,B', help='what to call the two in the report')
    ap.add_argument('--report')
    ap.add_argument('--child', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for tag, lib in (('a', args.a), ('b', args.b)):
            env = dict(os.environ)
            if lib:
                env['SG_LIB_PATH'] = os.path.abspath(lib)
            paths.append(os.path.join(tmp, tag + '.npz'))
            subprocess.run([sys.executable, os.path.abspath(__file__), '--child', paths[-1]], env=env, check=True, timeout=300)
        return compare(paths[0], paths[1], args.report, tuple(args.names.split(',')))


if __name__ == '__main__':
    sys.exit(main())
