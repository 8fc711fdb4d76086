"""Device time of the pyannote segmentation and diarization on synthetic audio: one 10 s window, `windows` at the 5 s step and `diarize`
on 10 min and 60 min (119 and 719 windows).  Writes one JSON line to profiles/seg_bench.json.  Synthetic weights (qasr.synth)."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "qwen3-asr-swift_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import pyannote_oracle as O
from qasr import synth
from qasr import diarization as D
from qasr.speaker import WeSpeakerModel


def main():
    d = tempfile.mkdtemp()
    synth.write_pyannote_safetensors(synth.synth_pyannote_state_dict(0), os.path.join(d, "seg"))
    synth.write_wespeaker_safetensors(synth.synth_wespeaker_state_dict(0), os.path.join(d, "spk"))
    seg = D.SegmentationModel.from_pretrained(os.path.join(d, "seg"))
    spk = WeSpeakerModel.from_pretrained(os.path.join(d, "spk"))
    pipe = D.PyannoteDiarizationPipeline.from_models(seg, spk)
    base = O.turns_clip(5, 60.0)
    out = {}
    one = base[:160000]
    seg.forward(one)
    ms = []
    for _ in range(5):
        seg.forward(one)
        ms.append(seg.timing())
    out["one_window_ms"] = round(min(ms), 3)
    for minutes in (10, 60):
        x = np.tile(base, minutes)
        seg.windows(x)
        pos, _, _, _ = seg.windows(x)
        t0 = time.perf_counter()
        r = pipe.diarize(x)
        wall = (time.perf_counter() - t0) * 1e3
        out[f"{minutes}min"] = {"windows": len(pos), "windows_device_ms": round(seg.timing(), 2), "diarize_wall_ms": round(wall, 1),
                                "embed_device_ms": round(spk.timing(), 2), "segments": len(r.segments), "speakers": r.num_speakers}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    line = json.dumps(out)
    open(os.path.join(ROOT, "profiles", "seg_bench.json"), "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
