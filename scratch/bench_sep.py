"""Device time of the Open-Unmix source separation on synthetic audio and weights: one 10 s clip, one 3 min file and a batch of 3 min
files (--batch, 32 by default), per stage from HIP events (qasr_sep_timing), and the microseconds per recurrent step of the streamed and
the resident + streamed recurrence forms at hidden 256 and 512 per direction (umxhq / umxl).  Writes one JSON line to
profiles/sep_bench.json.

Estimate written before the first measurement: a step streams the 1 MiB of W_hh (hidden 256) from L2 at about 200 GB/s per workgroup,
about 5 us; a 3 min file has 7752 frames x 3 layers, so about 120 ms of recurrence for any batch up to 4 files per (stem, direction)."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "qwen3-asr-swift_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import openunmix_oracle as O
from qasr import synth
from qasr.separation import SourceSeparator


def best(sep, clips, reps):
    sep.separate_batch(clips)
    rows = []
    for _ in range(reps):
        sep.separate_batch(clips)
        rows.append(sep.timing())
    return {k: round(min(r[k] for r in rows), 3) for k in rows[0]}


def step_us(sep, T, form):
    """Microseconds per recurrent step and layer: the network time of T frames minus that of T / 2 frames (one file, so the GEMMs' share
    of the difference is small next to the 3 x T / 2 dependent steps), and the network time at T."""
    sep.set_recurrence_form(form)
    mag = np.abs(np.random.default_rng(0).standard_normal((T, 2, 2049))).astype(np.float32)
    t = {}
    for n in (T, T // 2):
        sep.masks(mag[:n])
        ms = []
        for _ in range(3):
            sep.masks(mag[:n])
            ms.append(sep.timing()["network"])
        t[n] = min(ms)
    sep.set_recurrence_form(0)
    return round((t[T] - t[T // 2]) * 1e3 / (3 * (T - T // 2)), 3), round(t[T], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=2000)
    args = ap.parse_args()
    d = tempfile.mkdtemp()
    out = {"estimate_us_per_step_hidden256": 5.0, "estimate_recurrence_ms_3min": 120.0}
    hq = SourceSeparator.from_pretrained(synth.write_openunmix_safetensors(synth.synth_openunmix_state_dict(0, 512), os.path.join(d, "hq")),
                                         max_batch_samples=max(args.batch, 1) * 180 * 44100)
    base = O.clip(0, 10 * 44100)
    out["10s"] = best(hq, [base], 3)
    three = np.tile(base, 18)
    out["3min"] = best(hq, [three], 2)
    if args.batch > 1:
        out["%dx3min" % args.batch] = best(hq, [three] * args.batch, 1)
    for form, name in ((0, "streamed"), (1, "resident")):
        us, ms = step_us(hq, args.steps, form)
        out["hidden256_%s" % name] = {"us_per_step_and_layer": us, "network_ms": ms, "T": args.steps}
    hq.close()
    xl = SourceSeparator.from_pretrained(synth.write_openunmix_safetensors(synth.synth_openunmix_state_dict(0, 1024), os.path.join(d, "xl")))
    for form, name in ((0, "streamed"), (1, "resident")):
        us, ms = step_us(xl, args.steps // 2, form)
        out["hidden512_%s" % name] = {"us_per_step_and_layer": us, "network_ms": ms, "T": args.steps // 2}
    xl.close()
    out["recurrence_winner_hidden256"] = min(("streamed", "resident"), key=lambda n: out["hidden256_" + n]["us_per_step_and_layer"])
    out["recurrence_winner_hidden512"] = min(("streamed", "resident"), key=lambda n: out["hidden512_" + n]["us_per_step_and_layer"])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    line = json.dumps(out)
    open(os.path.join(ROOT, "profiles", "sep_bench.json"), "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
