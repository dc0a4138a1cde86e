# Gradient-clipping probe (needs a GPU; fails without one):
#   (a) ob_sqnorm_multi_f32 over GPT-2 small's 14 flat-grad sizes against
#       torch._foreach_norm over the same buffers, with bytes/time against
#       the measured 6.29 TB/s HBM copy rate;
#   (b) k_adamw (ob_adamw_step) against k_adamw_scaled on one 38.6 M-element
#       buffer (the final layer's size).
# Device events around every single call, warm-up, the two sides of each
# comparison alternating call by call.  The timed calls are split into 5
# equal repeats; a side's figure is the median over all its calls and its
# spread is max - min of its per-repeat medians.
# Writes the result as JSON (default profiles/grad_clip_probe.json).
import argparse
import ctypes
import json
import pathlib
import statistics
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oobleck_amd._ext import check, get_ext  # noqa: E402
from oobleck_amd.config import GPT2_SMALL  # noqa: E402
from oobleck_amd.params import layer_param_numel  # noqa: E402

HBM_COPY_TBS = 6.29
REPEATS = 5


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def alternate(fn_a, fn_b, iters, warmup):
    """Per-call device-event times (ms) of fn_a and fn_b, alternating."""
    for _ in range(warmup):
        fn_a()
        fn_b()
    torch.cuda.synchronize()
    times = ([], [])
    evs = [(torch.cuda.Event(True), torch.cuda.Event(True)) for _ in range(2)]
    for _ in range(iters):
        for side, fn in enumerate((fn_a, fn_b)):
            st, en = evs[side]
            st.record()
            fn()
            en.record()
            en.synchronize()
            times[side].append(st.elapsed_time(en))
    return times


def summarize(ms):
    per = len(ms) // REPEATS
    meds = [statistics.median(ms[i * per:(i + 1) * per])
            for i in range(REPEATS)]
    return {"median_us": statistics.median(ms) * 1e3,
            "repeat_medians_us": [m * 1e3 for m in meds],
            "spread_us": (max(meds) - min(meds)) * 1e3,
            "calls": len(ms)}


def probe_sqnorm(ext, iters, warmup):
    mc = GPT2_SMALL
    sizes = [layer_param_numel(mc, mc.layer_kind(i))
             for i in range(mc.n_layers_total)]
    g = torch.Generator(device="cuda").manual_seed(0)
    bufs = [torch.randn(n, device="cuda", generator=g) * 3e-2 for n in sizes]
    n = len(bufs)
    ptrs = (ctypes.c_void_p * n)(*[b.data_ptr() for b in bufs])
    counts = (ctypes.c_int64 * n)(*sizes)
    ws = torch.empty(max(1, ext.ob_sqnorm_ws_count(counts, n)),
                     dtype=torch.float64, device="cuda")
    out = torch.zeros(n, dtype=torch.float64, device="cuda")

    def ours():
        check(ext.ob_sqnorm_multi_f32(ptrs, counts, None, n, vp(ws), vp(out),
                                      stream()), "sqnorm")

    def theirs():
        torch._foreach_norm(bufs)

    t_ours, t_torch = alternate(ours, theirs, iters, warmup)
    ref = torch.stack([x.double().pow(2).sum() for x in bufs])
    rel = ((out - ref).abs() / ref).max().item()
    nbytes = 4 * sum(sizes)
    res = {"tensors": n, "elements": sum(sizes), "bytes": nbytes,
           "max_rel_err_vs_torch_f64": rel,
           "ob_sqnorm_multi_f32": summarize(t_ours),
           "torch_foreach_norm": summarize(t_torch)}
    for k in ("ob_sqnorm_multi_f32", "torch_foreach_norm"):
        tbs = nbytes / (res[k]["median_us"] * 1e-6) / 1e12
        res[k]["TB_per_s"] = tbs
        res[k]["share_of_hbm_copy_rate"] = tbs / HBM_COPY_TBS
    return res


def probe_adamw(ext, iters, warmup):
    mc = GPT2_SMALL
    n = layer_param_numel(mc, mc.layer_kind(mc.n_layers_total - 1))
    g = torch.Generator(device="cuda").manual_seed(1)
    p = torch.randn(n, device="cuda", generator=g) * 0.02
    grad = torch.randn(n, device="cuda", generator=g) * 1e-2
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    stats = torch.tensor([1.0, 1.0, 0.5, 0.0], dtype=torch.float64,
                         device="cuda")
    hp = (1, 5e-5, 0.9, 0.999, 1e-8, 0.0)

    def plain():
        check(ext.ob_adamw_step(vp(p), vp(grad), vp(m), vp(v), n, *hp,
                                stream()), "adamw")

    def scaled():
        check(ext.ob_adamw_step_scaled(vp(p), vp(grad), vp(m), vp(v), n, *hp,
                                       vp(stats), stream()), "adamw_scaled")

    t_plain, t_scaled = alternate(plain, scaled, iters, warmup)
    nbytes = 28 * n
    res = {"elements": n, "bytes": nbytes, "k_adamw": summarize(t_plain),
           "k_adamw_scaled": summarize(t_scaled)}
    for k in ("k_adamw", "k_adamw_scaled"):
        res[k]["TB_per_s"] = nbytes / (res[k]["median_us"] * 1e-6) / 1e12
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" /
                                         "grad_clip_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_probe needs a GPU")
    assert args.iters >= REPEATS and args.iters % REPEATS == 0
    ext = get_ext()
    result = {"device": torch.cuda.get_device_name(0),
              "iters_per_side": args.iters, "warmup": args.warmup,
              "hbm_copy_rate_TB_per_s": HBM_COPY_TBS,
              "sqnorm_gpt2_small": probe_sqnorm(ext, args.iters, args.warmup),
              "adamw_final_layer": probe_adamw(ext, args.iters, args.warmup)}
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
