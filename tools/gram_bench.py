"""Timing of the Gram-matrix style loss (csrc/gram_loss.hip) on the GPU: profiles/gram_loss.md.

  taps     forward and backward of ``torch.ops.p2p.gram_loss_*`` at the five VGG19 tap shapes of a
           batch (default 64 x 256^2), and -- for comparison only -- ``torch.bmm`` on the same
           NHWC features (two Gram products forward, X D backward); the needed bytes and FLOPs
           come from the shapes.
  step     the reference-family step as a captured graph with ``lambda_style`` 0 and 1, the two
           taking turns inside every window.
  capture  a 64^2 step with ``lambda_style = 1``: K graph replays against K eager steps
           (deterministic mode), losses and state compared bitwise.

Device events around windows of calls after a warm-up; every figure is ms per call, one per window.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import p2p_pytorch_amd as p2p  # noqa: E402

TAPS = ((64, 1), (128, 2), (256, 4), (512, 8), (512, 16))     # (C, downscale) of relu1_1 .. relu5_1


def windows(fns, calls, nwin, warmup):
    """ms per call of each fn: ``nwin`` windows, the fns taking turns inside every window."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(nwin):
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                f()
            e1.record()
            e1.synchronize()
            out[i].append(e0.elapsed_time(e1) / calls)
    return out


def feats(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.relu(torch.randn(*shape, device="cuda", generator=g))
    return x.bfloat16().contiguous(memory_format=torch.channels_last)


def taps(args):
    from p2p_pytorch_amd.ops import hip
    P = hip.P()                                  # loads the extension: torch.ops.p2p
    one = torch.ones(1, device="cuda")
    for C, s in TAPS:
        B, H = args.batch, args.size // s
        N = H * H
        fx, fy = feats((B, C, H, H), 1), feats((B, C, H, H), 2)
        loss, _, dh = P.gram_loss_fwd(fx, fy)
        X, Y = (f.permute(0, 2, 3, 1).reshape(B, N, C) for f in (fx, fy))       # views of the NHWC memory
        D = dh.clone()
        t = windows([lambda: P.gram_loss_fwd(fx, fy), lambda: P.gram_loss_bwd(fx, dh, one),
                     lambda: (torch.bmm(X.transpose(1, 2), X), torch.bmm(Y.transpose(1, 2), Y)),
                     lambda: torch.bmm(X, D)], args.calls, args.windows, args.warmup)
        row = {"tap": f"{B}x{C}x{H}x{H}", "loss": loss.item(),
               "fwd_ms": t[0], "bwd_ms": t[1], "bmm_fwd_ms": t[2], "bmm_bwd_ms": t[3],
               # needed: both feature maps read once / fx read and dX written; upper-triangle FLOPs forward
               "fwd_bytes": 2 * B * N * C * 2, "bwd_bytes": 2 * B * N * C * 2,
               "fwd_flops": 2 * B * N * C * (C + 32), "bwd_flops": 2 * B * N * C * C}
        print(json.dumps(row), flush=True)


def _step(lam, batch, size, seed=7):
    from p2p_pytorch_amd.engine.compress_gan import CompressGANStep
    from p2p_pytorch_amd.models import VGGLoss, define_C, define_D, define_G
    from p2p_pytorch_amd.ops import hip
    dev = torch.device("cuda")
    hip.reset_rng(0)
    torch.manual_seed(seed)
    nets = (define_G(gpu_id=dev, verbose=False), define_D(6, 64, gpu_id=dev, verbose=False),
            define_C(gpu_id=dev, verbose=False))
    step = CompressGANStep(*nets, vgg=VGGLoss().to(dev), c_phase_backward=True, lambda_style=lam)
    g = torch.Generator(device=dev).manual_seed(5)
    data = [[(torch.rand(batch, 3, size, size, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
             .contiguous(memory_format=torch.channels_last) for _ in range(2)] for _ in range(3)]
    return step, nets, data


def step(args):
    from p2p_pytorch_amd.engine.graph import CapturedStep
    caps = []
    for lam in (0.0, 1.0):
        st, _, data = _step(lam, args.batch, args.size)
        caps.append((CapturedStep(st.step, *data[0], warmup=2), data[0]))     # raises CaptureError on failure
    t = windows([lambda c=c, d=d: c(*d) for c, d in caps], args.calls, args.windows, args.warmup)
    print(json.dumps({"step": f"{args.batch}x3x{args.size}x{args.size}", "captured": True,
                      "style_off_ms": t[0], "style_on_ms": t[1]}), flush=True)


def capture(args):
    from p2p_pytorch_amd.engine.graph import CapturedStep

    def state(nets):
        return torch.cat([p.detach().reshape(-1).float() for m in nets for p in m.parameters()] +
                         [b.detach().reshape(-1).float() for m in nets for b in m.buffers()
                          if b.dtype.is_floating_point])
    p2p.set_deterministic(True)
    st, nets, data = _step(1.0, 2, 64)
    for a, b in data:
        le = st.step(a, b)
    torch.cuda.synchronize()
    se, le = state(nets), {k: v.item() for k, v in le.items()}
    st, nets, data = _step(1.0, 2, 64)
    cap = CapturedStep(st.step, *data[0], warmup=2)
    for a, b in data:
        lg = cap(a, b)
    torch.cuda.synchronize()
    sg, lg = state(nets), {k: v.item() for k, v in lg.items()}
    p2p.set_deterministic(False)
    print(json.dumps({"capture": "2x3x64x64", "replays": len(data), "losses_equal": le == lg,
                      "state_equal": bool(torch.equal(se, sg)), "Style": lg["Style"]}), flush=True)
    assert le == lg and torch.equal(se, sg)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["taps", "step", "capture"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gram_bench: needs the GPU")      # no CPU fall-back: a CPU time says nothing
    p2p.set_backend("native")
    {"taps": taps, "step": step, "capture": capture}[args.what](args)
