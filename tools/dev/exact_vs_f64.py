"""precision="exact" against precision="f64" of ONE build on ONE set of frames: the first-pass fields of both on the same
tensors, rendered once, with the SHA-256 of those frames in front -- two runs are comparable only when their hashes agree
(profiles/exact_offsets/: the "offsets" of the exact first pass once recorded were frames rendered again between the runs).

    python tools/dev/exact_vs_f64.py [--pairs 64] [--size 2048] [--ws 64] [--kind wavy] [--noise 2.0] [--save DIR]

Prints: the hash of the frames and of either precision's fields, the windows that differ in any bit, the windows beyond
1e-11 px, the worst |du| and |dv|, the validity flags that differ, the windows that took the float64 transform.  Exits 1 when
a window lies beyond 1e-11 px or a flag differs; with --save their pixels go to DIR/beyond.npz (arrays a, b [n, ws, ws],
pair_row_col, u_exact, v_exact, u_f64, v_f64).
"""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from torchpiv_amd import engine, synth

TOL = 1e-11


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--ws", type=int, default=64)
    ap.add_argument("--kind", default="wavy")
    ap.add_argument("--noise", type=float, default=2.0)
    ap.add_argument("--save", default=None, metavar="DIR")
    args = ap.parse_args()
    H, ws, ov, n = args.size, args.ws, args.ws // 2, args.pairs

    A, B = synth.make_batch(n, H, H, kind=args.kind, noise=args.noise, device="cuda")
    print(f"{n} pairs {H}^2, {ws}/{ov}, {args.kind}, noise {args.noise:g}")
    print(f"frames sha256 {sha(A, B)}")
    pe = engine.Plan(H, H, ws, ov, n_pass=1, max_batch=n, precision="exact")
    ue, ve, ie = (t.clone() for t in pe.run(A, B))
    n_fb = pe.exact_fallbacks()
    pe.close()
    pf = engine.Plan(H, H, ws, ov, n_pass=1, max_batch=n, precision="f64")
    uf, vf, i_f = (t.clone() for t in pf.run(A, B))
    pf.close()
    torch.cuda.synchronize()
    print(f"exact fields sha256 {sha(ue, ve, ie)}")
    print(f"f64 fields sha256 {sha(uf, vf, i_f)}")

    du, dv = (ue - uf).abs(), (ve - vf).abs()
    bits = (ue.view(torch.int64) != uf.view(torch.int64)) | (ve.view(torch.int64) != vf.view(torch.int64))
    beyond = ~((du <= TOL) & (dv <= TOL))                  # (a NaN on one side counts)
    flags = ie != i_f
    print(f"windows {ue.numel()}, differing in any bit {int(bits.sum())}, beyond {TOL:g} px {int(beyond.sum())}, "
          f"max |du| {float(du.max()):.3e} max |dv| {float(dv.max()):.3e}, flags differing {int(flags.sum())}, "
          f"through the float64 transform {n_fb}")
    bad = beyond | flags
    if bad.any():
        where = bad.nonzero().cpu().numpy()
        for k, r, c in where[:20]:
            print(f"  pair {k} window ({r}, {c}): exact ({float(ue[k, r, c])!r}, {float(ve[k, r, c])!r}, {int(ie[k, r, c])}) "
                  f"f64 ({float(uf[k, r, c])!r}, {float(vf[k, r, c])!r}, {int(i_f[k, r, c])})")
        if args.save:
            os.makedirs(args.save, exist_ok=True)
            st = ws - ov
            cut = lambda F: np.stack([F[k, r * st:r * st + ws, c * st:c * st + ws].cpu().numpy() for k, r, c in where])
            pick = lambda F: F[bad].cpu().numpy()
            np.savez_compressed(os.path.join(args.save, "beyond.npz"), a=cut(A), b=cut(B), pair_row_col=where,
                                u_exact=pick(ue), v_exact=pick(ve), u_f64=pick(uf), v_f64=pick(vf))
            print(f"  pixels of {len(where)} windows -> {os.path.join(args.save, 'beyond.npz')}")
        sys.exit(1)


if __name__ == "__main__":
    main()
