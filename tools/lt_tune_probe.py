# Tunes the benchmark's library GEMM shapes (GPT-2 small, microbatch 8 x
# 1024: 12 BLOCK keys + 3 FINAL keys) in a fresh process, through the same
# ob_gemm_lt_tune the layers call at create time, and writes the record:
# per key the shape and flags, top-1's and the chosen solution's index,
# kernel name, microseconds and TF, candidates tried and dropped, and the
# total wall time of tuning.  A BLOCK's weight grads are tuned as the layer
# tunes them, with WS_DW_A of its plan as the slab, so the record also holds
# every sliced pair (K-slices + fold) that was timed, the
# slice count the step would run and the milliseconds the pairs added.
#
#   python tools/lt_tune_probe.py [OUT.json]     (default profiles/lt_tune_table.json)
import json
import os
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from oobleck_amd._ext import (LT_SHAPE_NAMES, ObLayerDesc, check, get_ext,  # noqa: E402
                              layer_lt_shapes, layer_plan, lt_candidates,
                              lt_choice, lt_shape, lt_slices)
from oobleck_amd.config import GPT2_SMALL as MC  # noqa: E402

B, S = 8, 1024
NAMES = {1: ["qkv", "attnproj", "fc", "mlpproj", "dX_mlpproj", "dX_fc",
             "dX_attnproj", "dX_qkv", "dW_mlpproj", "dW_fc", "dW_attnproj",
             "dW_qkv"],
         2: ["lm_head", "d_lnout", "dW_lm"]}


def main():
    out = pathlib.Path(sys.argv[1]) if len(sys.argv) > 1 else \
        ROOT / "profiles" / "lt_tune_table.json"
    torch.cuda.init()
    torch.zeros(1, device="cuda:0")
    ext = get_ext()
    rows = []
    t_all = time.perf_counter()
    for kind in (1, 2):
        d = ObLayerDesc(kind=kind, n_embd=MC.n_embd, n_head=MC.n_head,
                        n_positions=MC.n_positions, vocab_size=MC.vocab_size,
                        max_batch=B, seq_len=S, n_slots=1, dtype=1)
        shapes = layer_lt_shapes(d)
        assert len(shapes) == len(NAMES[kind]), shapes
        slab = layer_plan(d)["ws_dw_a"] if kind == 1 else 0
        for name, s in zip(NAMES[kind], shapes):
            check(ext.ob_gemm_lt_tune_slab(lt_shape(*s), slab if s[0] else 0),
                  "gemm_lt_tune_slab")
            c = lt_choice(s)
            if c is None:
                raise SystemExit("no table entry: is OB_LT_TUNE=0 set?")
            sd = dict(zip(LT_SHAPE_NAMES, s))
            flop = 2.0 * sd["M"] * sd["N"] * sd["K"]
            tf = lambda us: round(flop / us / 1e6, 1) if us > 0 else None  # noqa: E731
            rows.append({
                "name": name, "shape": sd, "tuned": c["tuned"],
                "top1": {"index": c["top1_index"], "kernel": c["top1_kernel"],
                         "us": round(c["us_top1"], 2), "tf": tf(c["us_top1"])},
                "chosen": {"index": c["index"], "kernel": c["chosen_kernel"],
                           "us": round(c["us_chosen"], 2),
                           "tf": tf(c["us_chosen"])},
                "top1_spread_us": round(c["spread_top1"], 2),
                "fastest": [{"index": t["index"], "list_pos": t["pos"],
                             "us": round(t["us"], 2)}
                            for t in lt_candidates(s)[:5]],
                "tried": c["tried"], "dropped": c["dropped"],
                "tune_wall_ms": round(c["wall_ms"], 1)})
            r = rows[-1]
            sl = lt_slices(s)
            if sl and sl["pairs"]:
                r["sliced"] = {
                    "slices": sl["slices"], "index": sl["slice_index"],
                    "fastest_pair_us": round(sl["us_sliced"], 2),
                    "fastest_pair_tf": tf(sl["us_sliced"]),
                    "added_tune_ms": round(sl["added_ms"], 1),
                    "pairs": [{"slices": q["slices"], "index": q["index"],
                               "us": round(q["us"], 2)} for q in sl["pairs"]]}
            print(f"{name:12s} top1 #{r['top1']['index']} {r['top1']['us']:9.1f} us "
                  f"{r['top1']['tf']} TF -> #{r['chosen']['index']} "
                  f"{r['chosen']['us']:9.1f} us {r['chosen']['tf']} TF  "
                  f"tried {r['tried']} dropped {r['dropped']} "
                  f"{r['tune_wall_ms']:.0f} ms", flush=True)
            if "sliced" in r:
                q = r["sliced"]
                print(f"{'':12s} sliced: " + ", ".join(
                    f"s={x['slices']} #{x['index']} {x['us']:.1f} us"
                    for x in q["pairs"]) +
                    f" -> runs {q['slices']} slice(s), "
                    f"+{q['added_tune_ms']:.0f} ms", flush=True)
    total = time.perf_counter() - t_all
    rec = {"model": "gpt2", "microbatch": B, "seq_len": S,
           "candidates_asked": int(os.environ.get("OB_LT_TUNE_N", "8")),
           "all_algos": os.environ.get("OB_LT_TUNE_ALL", "0")[:1] == "1",
           "dw_slices": os.environ.get("OB_DW_SLICES", "0"),
           "sliced_added_tune_ms": round(sum(
               r["sliced"]["added_tune_ms"] for r in rows if "sliced" in r), 1),
           "device": torch.cuda.get_device_name(0),
           "total_tune_wall_s": round(total, 2), "keys": rows}
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(f"total tuning wall time {total:.2f} s -> {out}")


if __name__ == "__main__":
    main()
