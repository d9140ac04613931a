"""Regenerates tests/golden/lbs_weights_params.npz and lbs_weights_<case>.npz from the reference's own module:

    python tests/golden/make_golden_lbs_weights.py <MOSS checkout>

``CrossAttention_lbs`` (nets/mlp_delta_weight_lbs.py) is imported from the checkout and run on the CPU in float64 and in float32
(``Tensor.cuda`` is the identity for the duration: the module calls it on a constant).  Cases:

* ``init``  -- the module as constructed, P = 797 (a prime: no multiple of any tile);
* ``sharp`` -- the same state with ``query.*`` and ``key.*`` multiplied by 4 (exact in float32: the attention stops being
  near-uniform), P = 1100.

x is uniform in +-1, Rs are rotations from axis-angles of scale 0.4, the cotangent g (1,P,24) is standard normal.  Stored per case:
``out`` (float64), the gradients of <out, g> w.r.t. x, Rs and the 16 parameters the forward reads (float64 autograd, rounded once to
float32), beside each result X ``X_err32`` = the largest absolute difference between the reference's float32 run and its float64
run, and a SHA-256 of the inputs.  The parameters (all 20 tensors of the state_dict) are stored once, in lbs_weights_params.npz.

No point sits near a ReLU kink: a float32 pre-activation on the other side of zero than its float64 value changes that point's
gradient discontinuously (the reference's own float32 run does it).  So the generator measures the largest float32 pre-activation
error over its candidate points (``preact_err32``, stored), and keeps only candidates whose 512 float64 pre-activations all have
|z| >= 16 * preact_err32 (twice the tests' parity factor 8).  Nothing is excluded at test time.
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
USED = tuple(f"{m}.{w}" for m in ("bw_linears.0", "bw_linears.1", "bw_linears.2", "bw_linears.3", "bw_fc", "query", "key", "value")
             for w in ("weight", "bias"))
CASES = {"init": dict(P=797, seed=11, scale=1.0), "sharp": dict(P=1100, seed=12, scale=4.0)}
KINK_FACTOR = 16.0


def rotations(rng, n, scale):
    r = rng.normal(size=(n, 3)) * scale
    th = np.linalg.norm(r, axis=1)[:, None, None]
    k = r / th[:, :, 0]
    Kx = np.zeros((n, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return (np.eye(3)[None] + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx).astype(np.float32)


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float32)).tobytes())
    return h.hexdigest()


def main(checkout):
    sys.path.insert(0, checkout)
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        from nets.mlp_delta_weight_lbs import CrossAttention_lbs, xyz_embedder
        torch.manual_seed(20240607)
        base = CrossAttention_lbs()
        state0 = {k: v.detach().clone() for k, v in base.state_dict().items()}
        assert len(state0) == 20 and all(k in state0 for k in USED)
        np.savez(os.path.join(HERE, "lbs_weights_params.npz"), **{k: v.numpy() for k, v in state0.items()})

        def module(state, dtype):
            net = CrossAttention_lbs().to(dtype)
            net.load_state_dict({k: v.to(dtype) for k, v in state.items()})
            return net

        def preacts(net, x):
            f = xyz_embedder(x[None]).permute(0, 2, 1)
            h, zs = f, []
            for i, layer in enumerate(net.bw_linears):
                z = layer(h)
                zs.append(z)
                h = torch.relu(z)
                if i in net.skips:
                    h = torch.cat((f, h), 1)
            return torch.cat(zs, 1)[0]                      # (512, P)

        def run(net, x, Rs, g):
            x = x.clone().requires_grad_(True)
            Rs = Rs.clone().requires_grad_(True)
            out = net(x[None], Rs)
            params = dict(net.named_parameters())
            grads = torch.autograd.grad((out * g).sum(), [x, Rs] + [params[k] for k in USED])
            assert all(params[k].grad is None for k in params)
            return out.detach(), dict(zip(("x", "Rs") + USED, grads))

        for case, cfg in CASES.items():
            rng = np.random.default_rng(cfg["seed"])
            state = {k: (v * cfg["scale"] if k.split(".")[0] in ("query", "key") else v.clone()) for k, v in state0.items()}
            n64, n32 = module(state, torch.float64), module(state, torch.float32)
            cand = torch.from_numpy(rng.uniform(-1, 1, size=(2 * cfg["P"], 3)).astype(np.float32))
            with torch.no_grad():
                z64, z32 = preacts(n64, cand.double()), preacts(n32, cand)
            preact_err32 = float((z32.double() - z64).abs().max())
            keep = z64.abs().min(0).values >= KINK_FACTOR * preact_err32
            assert int(keep.sum()) >= cfg["P"], "too few candidates away from every kink"
            x = cand[keep][:cfg["P"]].contiguous()
            Rs = torch.from_numpy(rotations(rng, 23, 0.4))
            g = torch.from_numpy(rng.normal(size=(1, cfg["P"], 24)).astype(np.float32))
            with torch.no_grad():
                assert bool(((preacts(n32, x) > 0) == (preacts(n64, x.double()) > 0)).all())
            out64, gr64 = run(n64, x.double(), Rs.double(), g.double())
            out32, gr32 = run(n32, x, Rs, g)
            rec = {"x": x.numpy(), "Rs": Rs.numpy(), "g": g.numpy(), "param_scale": np.float32(cfg["scale"]),
                   "preact_err32": np.float64(preact_err32), "rejected_share": np.float64(1.0 - float(keep.float().mean())),
                   "out": out64.numpy(), "out_err32": np.float64(float((out32.double() - out64).abs().max())),
                   "inputs_sha256": sha([x.numpy(), Rs.numpy(), g.numpy()] + [state[k].numpy() for k in USED])}
            for k in gr64:
                rec[f"grad_{k}"] = gr64[k].numpy().astype(np.float32)
                rec[f"grad_{k}_err32"] = np.float64(float((gr32[k].double() - gr64[k]).abs().max()))
            np.savez(os.path.join(HERE, f"lbs_weights_{case}.npz"), **rec)
            print(case, "P", cfg["P"], "preact_err32 %.3g" % preact_err32, "rejected %.3f" % rec["rejected_share"],
                  "out spread %.3g" % float(out64.std(1).max()), "out_err32 %.3g" % rec["out_err32"])
    finally:
        torch.Tensor.cuda = real_cuda


if __name__ == "__main__":
    main(sys.argv[1])
