"""Mints tests/golden/segment_ref.json from the reference's EXECUTED code: its segment/silero_vad.py is imported by file path,
``SileroVADSegmenter`` is built through ``object.__new__`` (its ``__init__`` downloads a model with ``torch.hub``) and its ``pdac``,
``get_speech_timestamps`` (with a stub model that replays a probability track) and ``segment_long_input`` run on seeded tracks.
The JSON holds the tracks and the results; tests/test_segment_cpu.py reads only the JSON.

    python tests/golden/make_segment_goldens.py <reference tree>/src/seamless_communication
"""
from __future__ import annotations

import importlib.util
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
OUT = HERE / "segment_ref.json"
WINDOW = 1536
RATE = 16000


class ReplayModel:
    """what get_speech_probs asks of a Silero model: reset_states(), parameters() and one probability per chunk"""

    def __init__(self, probs):
        self.probs = list(probs)
        self.pos = 0

    def reset_states(self):
        self.pos = 0

    def parameters(self):
        return iter([torch.zeros(1)])

    def __call__(self, chunk, sampling_rate):
        assert chunk.shape == (WINDOW,) and sampling_rate == RATE
        self.pos += 1
        return torch.tensor(self.probs[self.pos - 1])


def track(rng, pieces):
    """pieces: (speech?, windows) -> probabilities, speech in (0.55, 0.99), the rest in (0.01, 0.45)"""
    out = []
    for speech, n in pieces:
        out += list(rng.uniform(0.55, 0.99, n) if speech else rng.uniform(0.01, 0.45, n))
    return np.asarray(out, dtype=np.float64)


def random_pieces(rng, total):
    pieces, speech, left = [], bool(rng.integers(2)), total
    while left > 0:
        n = int(min(left, rng.integers(2, 60) if speech else rng.integers(1, 25)))
        pieces.append((speech, n))
        speech, left = not speech, left - n
    return pieces


def main():
    ref_root = Path(sys.argv[1])
    spec = importlib.util.spec_from_file_location("ref_silero_vad", ref_root / "segment" / "silero_vad.py")
    ref = importlib.util.module_from_spec(spec)
    sys.modules["ref_silero_vad"] = ref
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(20241020)
    S, N = True, False
    plans = [
        # (name, pieces, chunk_size_sec, pause_length)
        ("islands_in_silence", [(N, 20), (S, 40), (N, 30), (S, 25), (N, 12), (S, 60), (N, 40), (S, 30), (N, 43)], 10, .5),
        ("islands_in_silence_chunk2", [(N, 20), (S, 40), (N, 30), (S, 25), (N, 12), (S, 60), (N, 13)], 2, .5),
        ("nothing_above_half_short", [(N, 5)], 10, .5),
        ("nothing_above_half", [(N, 150)], 10, .5),
        ("nothing_above_half_chunk20", [(N, 400)], 20, 1),
        ("all_above_half_short", [(S, 5)], 10, .5),
        ("all_above_half", [(S, 150)], 10, .5),
        ("all_above_half_chunk2", [(S, 400)], 2, .5),
        ("one_long_island", [(N, 10), (S, 350), (N, 10)], 10, .5),
        ("one_long_island_chunk2", [(N, 10), (S, 180), (N, 10)], 2, .5),
        ("one_long_island_chunk20", [(N, 3), (S, 390), (N, 7)], 20, 1),
        ("islands_below_min_duration", [(N, 15), (S, 3), (N, 20), (S, 5), (N, 18), (S, 4), (N, 30), (S, 2), (N, 25), (S, 5), (N, 73)], 10, .5),
        ("islands_below_min_duration_chunk2", [(N, 9), (S, 3), (N, 8), (S, 5), (N, 7), (S, 30), (N, 6), (S, 4), (N, 28)], 2, .5),
        # 0.5 s are 5.2 windows, 1 s are 10.4: pauses of 5 / 6 and of 10 / 11 windows lie on either side
        ("pauses_around_half_a_second", [(S, 12), (N, 5), (S, 12), (N, 6), (S, 12), (N, 5), (S, 12), (N, 6), (S, 12), (N, 30), (S, 12)], 2, .5),
        ("pauses_around_one_second", [(S, 30), (N, 10), (S, 30), (N, 11), (S, 30), (N, 10), (S, 30), (N, 11), (S, 30), (N, 150), (S, 28)], 10, 1),
        ("pauses_chunk20", [(S, 100), (N, 10), (S, 100), (N, 11), (S, 100), (N, 10), (S, 69)], 20, 1),
    ]
    for i, (total, chunk, pause) in enumerate([(7, 2, .5), (60, 2, .5), (120, 2, .5), (250, 10, .5), (400, 10, 1), (400, 20, 1), (333, 20, .5)]):
        plans.append((f"random_{i}", random_pieces(rng, total), chunk, pause))
    cases = []
    for name, pieces, chunk, pause in plans:
        probs = track(rng, pieces)
        assert len(set(probs.tolist())) == len(probs), "two equal values: the stable order and the reference's could differ"
        assert 5 <= len(probs) <= 400
        seg = object.__new__(ref.SileroVADSegmenter)
        seg.sample_rate, seg.chunk_size_sec, seg.pause_length = RATE, chunk, pause
        seg.model = ReplayModel(probs)
        max_len, min_len = chunk * RATE, 500 / 1000 * RATE
        pdac = [[int(s.start), int(s.end)] for s in seg.pdac(probs, max_len, min_len, WINDOW)]
        audio = torch.zeros(len(probs) * WINDOW - 100)  # the last chunk is padded
        stamps = [[int(a), int(b)] for a, b in seg.get_speech_timestamps(audio, seg.model, sampling_rate=RATE)]
        assert stamps == pdac
        long_input = [[int(a), int(b)] for a, b in seg.segment_long_input(audio)]
        cases.append({"name": name, "chunk_size_sec": chunk, "pause_length": pause, "window": WINDOW, "sample_rate": RATE,
                      "audio_samples": int(audio.shape[0]), "probs": probs.tolist(), "pdac": pdac, "speech_timestamps": stamps,
                      "segment_long_input": long_input})
        print(f"{name:36s} windows {len(probs):4d} chunk {chunk:2d} pdac {len(pdac):3d} segments {len(long_input):3d}")
    OUT.write_text(json.dumps({"cases": cases}, indent=0) + "\n")
    print("wrote", OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
