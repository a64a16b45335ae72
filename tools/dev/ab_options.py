"""Do two trees check the keywords alike?  (one-off aid for changes of the host layer that must not move a message)
   python tools/dev/ab_options.py dump out.json [tree]   -> every case's result or exception of the tree (default: this one)
   python tools/dev/ab_options.py cmp a.json b.json       -> the cases that differ; those of the group "multi" -- calls with
                                                             more than one fault, whose precedence may differ -- apart
Needs no GPU: Plan / ResidentPIV run up to the point where they ask for one.  Results are written as repr, tensors and
arrays as dtype, shape and a hash of their bytes, exceptions as class name and message."""
import hashlib, inspect, itertools, json, os, re, sys, tempfile

PARSERS = ("correlation_arg", "weighting_arg", "outlier_arg", "uncertainty_arg", "mask_arg", "dynamic_mask_arg", "prefilter_arg",
           "equalize_arg", "depth_arg", "dewarp_arg", "deform_arg", "derive_arg")
HOST_TESTS = ("background", "deform", "depth", "derive", "dewarp", "dynmask", "ensemble", "equalize", "frame_chain", "mask", "outlier",
              "phase", "prefilter", "uncertainty", "weighting")                 # tests/test_<name>_host.py
FEATURES = {"uncertainty": "cs", "deform": 2, "ensemble": True, "correlation": "rpc", "weighting": "gaussian",
            "dynamic_mask": {"kind": "bright", "size": 5, "level": 200}}
MODES = ("CWS", "DWS", "CWS_Fast")
CHAINS = ((32,), (64, 32, 16), (32, 16, 8), (48,), (128,))
H = W = 256


def describe(x):
    import numpy as np
    import torch
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous()
        return f"tensor({x.dtype}, {tuple(x.shape)}, {hashlib.sha1(x.view(torch.uint8).numpy().tobytes()).hexdigest()[:12]})"
    if isinstance(x, np.ndarray):
        return f"array({x.dtype}, {x.shape}, {hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest()[:12]})"
    if isinstance(x, dict):
        return "{" + ", ".join(f"{k!r}: {describe(v)}" for k, v in x.items()) + "}"
    if isinstance(x, (list, tuple)):
        return ("[%s]" if isinstance(x, list) else "(%s)") % ", ".join(describe(v) for v in x)
    return re.sub(r" at 0x[0-9a-f]+", "", repr(x))


def outcome(f, *args, **kw):
    try:
        return describe(f(*args, **kw))
    except Exception as e:                                              # noqa: BLE001 -- the exception is the result
        return f"{type(e).__name__}: {e}"


def subsets(names):
    return [dict((k, FEATURES[k]) for k in c) for r in range(len(names) + 1) for c in itertools.combinations(names, r)]


def dump(path, tree):
    sys.path.insert(0, tree)
    os.chdir(tree)
    import numpy as np
    import pytest
    import torch
    from torchpiv_amd import backend, engine
    out = {}

    # 1. the parsers: what the host tests feed them themselves (recorded while those tests run; what the constructors pass
    # on differs from tree to tree and is groups 2 to 4's business), then variations of it
    homes = [engine] + ([sys.modules["torchpiv_amd.options"]] if "torchpiv_amd.options" in sys.modules else [])
    plain = {name: getattr(engine, name) for name in PARSERS}
    seen = {name: [] for name in PARSERS}

    def recorder(name):
        def call(*args, **kw):
            if os.sep + "tests" + os.sep in sys._getframe(1).f_code.co_filename:
                seen[name].append((args, kw))
            return plain[name](*args, **kw)
        return call
    for name in PARSERS:
        for m in homes:
            setattr(m, name, recorder(name))
    rc = pytest.main(["-q", "-m", "not gpu", "-p", "no:cacheprovider"] + [f"tests/test_{t}_host.py" for t in HOST_TESTS])
    for name in PARSERS:
        for m in homes:
            setattr(m, name, plain[name])
    scalars = [True, np.bool_(True), np.int64(3), np.float32(0.5), float("nan"), float("inf"), float("-inf"), 3, 0.5, "x", (1, 2)]
    for name in PARSERS:
        calls = list(seen[name])
        keys = sorted({k for a, _ in calls if a and isinstance(a[0], dict) for k in a[0] if isinstance(k, str)})
        good = [a[0] for a, kw in calls if a and isinstance(a[0], dict) and not kw and not outcome(plain[name], *a).startswith("ValueError")]
        for a, kw in list(calls):
            try:
                calls.append(((plain[name](*a, **kw),), {}))             # its own result, fed back in
            except Exception:                                           # noqa: BLE001
                pass
        calls += [((v,), {}) for v in scalars + [{}]]
        calls += [(({k: v},), {}) for k in keys for v in scalars]
        calls += [((dict(g, **{k: v}),), {}) for g in good[:3] for k in keys for v in scalars]
        for a, kw in calls:
            out[f"parser/{name}({describe(a)}, {describe(kw)})"] = outcome(plain[name], *a, **kw)

    # 2. Plan and ResidentPIV on CPU tensors, every subset of the features each takes, x modes x size chains
    frames = torch.zeros(2, H, W, dtype=torch.uint8)
    for mode, chain in itertools.product(MODES, CHAINS):
        for kw in subsets(("uncertainty", "deform", "ensemble", "correlation", "weighting")):
            out[f"plan/{mode} {chain} {sorted(kw)}"] = outcome(
                engine.Plan, H, W, chain[0], chain[0] // 2, n_pass=len(chain), mode=mode, **kw)
        for kw in subsets(("uncertainty", "deform", "correlation", "weighting", "dynamic_mask")):
            out[f"resident/{mode} {chain} {sorted(kw)}"] = outcome(
                backend.ResidentPIV, frames, frames, chain[0], chain[0] // 2, multipass=len(chain), multipass_mode=mode, **kw)

    # 3. ensemble() of an object against every subset of what it may hold
    def bare(chain, kw):
        par = {k: getattr(engine, k + "_arg")(v) for k, v in kw.items()}
        piv = backend.ResidentPIV.__new__(backend.ResidentPIV)
        if len(inspect.signature(piv._init_state).parameters) > 5:       # the tree with one positional argument per keyword
            piv._init_state(torch.device("cpu"), range(2), None, chain[0], chain[0] // 2, len(chain), "CWS", 1, 1.0, 2.0,
                            "exact", 1.2, 3, None, None, **par)
        else:
            from torchpiv_amd import options
            run = dict(wind_size=chain[0], overlap=chain[0] // 2, multipass=len(chain), multipass_mode="CWS", dt=1, scale=1.0,
                       multipass_scale=2.0, precision="exact", validation_ratio=1.2, validation_window=3)
            piv._init_state(torch.device("cpu"), range(2), None, run, options.Options(**par))
        return piv._ensemble_check()
    for chain in CHAINS:
        for kw in subsets(("uncertainty", "deform", "correlation", "weighting", "dynamic_mask")):
            out[f"ensemble_check/{chain} {sorted(kw)}"] = outcome(bare, chain, kw)

    # 4. the constructors with one fault, and ("multi") with more than one: the precedence between the faults
    empty = tempfile.mkdtemp()

    def offline(device="cuda:0", folder=empty, **kw):
        return backend.OfflinePIV(folder, device, "bmp", 32, 16, **kw)

    def resident(a=frames, b=frames, **kw):
        return backend.ResidentPIV(a, b, 32, 16, **kw)
    bad = {"background": "x", "outlier": "x", "depth": "x", "mask": 5, "dewarp": "x", "uncertainty": "x", "derive": "x",
           "deform": "x", "correlation": "x", "weighting": "x", "dynamic_mask": "x", "equalize": "x", "prefilter": "x", "precision": "x"}
    small = np.zeros((8, 8), np.uint8)
    for k, v in bad.items():
        out[f"single/offline {k}"] = outcome(offline, **{k: v})
        out[f"single/resident {k}"] = outcome(resident, **{k: v})
    out["single/offline device"] = outcome(offline, device="nope")
    out["single/resident uint16 frames"] = outcome(resident, frames.to(torch.uint16), frames.to(torch.uint16))
    for k, v in {"background": small, "mask": small, "dewarp": {"map": (small, small)}, "dynamic_mask": {"stack": small[None]}}.items():
        out[f"single/resident shape of {k}"] = outcome(resident, **{k: v})
    for a, b in itertools.combinations(bad, 2):
        out[f"multi/offline {a} + {b}"] = outcome(offline, **{a: bad[a], b: bad[b]})
        out[f"multi/resident {a} + {b}"] = outcome(resident, **{a: bad[a], b: bad[b]})
    for k in bad:
        out[f"multi/offline device + {k}"] = outcome(offline, device="nope", **{k: bad[k]})
        out[f"multi/offline folder + {k}"] = outcome(offline, folder="/no/such/folder", **{k: bad[k]})
        out[f"multi/offline conflict + {k}"] = outcome(offline, **dict({"correlation": "rpc", "uncertainty": "cs"}, **{k: bad[k]}))
        out[f"multi/resident conflict + {k}"] = outcome(resident, **dict({"correlation": "rpc", "uncertainty": "cs"}, **{k: bad[k]}))
        if k in ("outlier", "mask", "uncertainty", "deform", "correlation", "weighting", "precision"):
            out[f"multi/plan conflict + {k}"] = outcome(engine.Plan, H, W, 32, 16, **dict({"ensemble": True, "deform": 2}, **{k: bad[k]}))
    os.rmdir(empty)
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    groups = {g: sum(k.startswith(g + "/") for k in out) for g in ("parser", "plan", "resident", "ensemble_check", "single", "multi")}
    print("dumped", len(out), "cases", groups, "of", tree, "to", path, "(host tests exit code", int(rc), ")")


def cmp(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    diff = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
    for k in diff:
        print(f"{k}\n    a: {a.get(k)}\n    b: {b.get(k)}")
    strict = [k for k in diff if not k.startswith("multi/")]
    print(f"{len(a)} / {len(b)} cases, {len(diff)} differ, {len(strict)} of them outside the group 'multi'")
    print("IDENTICAL" if not strict else "DIFFERENT")
    return 1 if strict else 0


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1] == "dump":
        dump(os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else here)
    else:
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
