"""Do two builds of the library produce the same BITS?  (development aid for changes that must not move a result)
   python tools/dev/ab_bits.py dump out.npz     (with TPIV_LIB=<build>)      -> fields of a fixed set of plans on seeded frames
   python tools/dev/ab_bits.py cmp a.npz b.npz                               -> per-array count of differing bytes
The dump holds the SHA-256 of every frame set it rendered ("in<tag>"); cmp first compares those and says INPUTS DIFFER for a
plan whose frames were not the same in the two runs -- its field counts then say nothing about the builds
(profiles/exact_offsets/)."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

CASES = [  # (H, W, ws, passes, mode, precision, kind, noise)
    (512, 512, 64, 2, "CWS", "exact", "wavy", 2.0), (512, 512, 64, 2, "DWS", "fast", "wavy", 2.0),
    (512, 512, 32, 3, "CWS", "fast", "wavy", 4.0), (512, 512, 32, 3, "DWS", "exact", "wavy", 4.0),
    (512, 768, 128, 2, "CWS", "fast", "wavy", 2.0), (384, 512, 16, 2, "CWS", "fast", "wavy", 6.0),
    (512, 512, 64, 1, "CWS", "fast", "wavy", 30.0), (256, 256, 32, 1, "CWS", "fast", "noise", 0.0),
    (512, 512, 48, 2, "CWS", "fast", "wavy", 2.0),
]
# the variant kernels (xcorr_variant.hpp), each chain in DWS and in CWS: 64 -> 32 -> 16 runs the pass-1 instance of 64 and the
# shifted instances of 32 and 16, 64 -> 64 the shifted instances of 64, and one single-pass plan each the pass-1 instances of
# 32 and 16
VARIANTS = {"phase": {"correlation": "phase"}, "rpc": {"correlation": "rpc"}, "gauss": {"weighting": "gaussian"},
            "ens": {"ensemble": True}}
CHAINS = [(64, 3, 2.0), (64, 2, 1.0), (32, 1, 2.0), (16, 1, 2.0)]      # (first window size, passes, pass_scale)
V_H = V_W = 512

if sys.argv[1] == "dump":
    import torch
    from torchpiv_amd import engine, synth
    out = {}

    def put(tag, u, v, inv):
        out["u" + tag], out["v" + tag], out["m" + tag] = u.cpu().numpy(), v.cpu().numpy(), inv.cpu().numpy()

    def put_inputs(tag, *frames):
        h = hashlib.sha256()
        for f in frames:
            h.update(f.contiguous().cpu().numpy().tobytes())
        out["in" + tag] = np.frombuffer(h.digest(), np.uint8)

    for i, (H, W, ws, n_pass, mode, prec, kind, noise) in enumerate(CASES):
        try:
            A, B = synth.make_batch(3, H, W, device="cuda", kind=kind, noise=noise)
        except Exception:                                           # noqa: BLE001 -- kinds this synth does not know
            g = torch.Generator(device="cuda").manual_seed(7 + i)
            A = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, device="cuda", generator=g)
            B = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, device="cuda", generator=g)
        put_inputs(str(i), A, B)
        plan = engine.Plan(H, W, ws, ws // 2, n_pass=n_pass, mode=mode, max_batch=3, precision=prec)
        put(str(i), *plan.run(A, B))
        torch.cuda.synchronize()
        plan.close()
    A, B = synth.make_batch(3, V_H, V_W, device="cuda", kind="wavy", noise=2.0)
    A2, B2 = synth.make_batch(3, V_H, V_W, device="cuda", kind="wavy", noise=5.0)      # the second ensemble_add
    A[0, :96, :96] = 0                                              # empty windows: zeroed in one frame, constant in both
    A[1, 128:224, 128:224] = 9
    B[1, 128:224, 128:224] = 9
    put_inputs("_variants", A, B, A2, B2)                           # one frame set for every variant chain
    n_plans = len(CASES)
    for name, kw in VARIANTS.items():
        for ws, n_pass, scale in CHAINS:
            for mode in ("DWS", "CWS"):
                if n_pass == 1 and mode == "DWS":
                    continue                                        # a single pass has no shifted pass: one plan is enough
                tag = f"_{name}_{ws}x{n_pass}s{scale:g}_{mode}"
                plan = engine.Plan(V_H, V_W, ws, ws // 2, n_pass=n_pass, mode=mode, max_batch=3, precision="fast", pass_scale=scale,
                                   **kw)
                if name == "ens":
                    for p in range(n_pass):
                        plan.ensemble_begin(p)
                        plan.ensemble_add(A, B)
                        plan.ensemble_add(A2, B2)
                        put(f"{tag}_p{p}", *plan.ensemble_end())
                    out["acc" + tag] = plan.ensemble_maps()[0].cpu().numpy()      # of the last pass
                else:
                    put(tag, *plan.run(A, B))
                torch.cuda.synchronize()
                plan.close()
                n_plans += 1
    np.savez(sys.argv[2], **out)
    print("dumped", n_plans, "plans,", len(out), "arrays to", sys.argv[2], "with", os.environ.get("TPIV_LIB", "the in-tree library"))
else:
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    bad = sorted(set(a.files) ^ set(b.files))
    if bad:
        print("arrays in one dump only:", bad)
    common = sorted(set(a.files) & set(b.files))
    inputs = [k for k in common if k.startswith("in")]
    if not inputs:
        print("no frame hashes in these dumps: whether the inputs were the same is not known")
    for k in inputs:                                                # before any field count
        if not np.array_equal(a[k], b[k]):
            bad.append(k)
            which = "every variant chain" if k == "in_variants" else "plan " + k[2:]
            print(f"INPUTS DIFFER for {which}: sha256 {a[k].tobytes().hex()} against {b[k].tobytes().hex()}")
    for k in common:
        if k in inputs:
            continue
        x, y = a[k], b[k]
        d = x.size if x.shape != y.shape or x.dtype != y.dtype else int((x.view(np.uint8) != y.view(np.uint8)).sum())
        if d:
            bad.append(k)
        print(f"{k:28s} differing bytes: {d} of {x.nbytes}  nan: {int(np.isnan(x).sum())}")
    print("IDENTICAL" if not bad else "DIFFERENT")
    sys.exit(1 if bad else 0)
