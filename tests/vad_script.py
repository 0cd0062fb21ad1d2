"""Scripts for the VAD stage (streaming/vad.py): the scenarios tests/golden/make_vad_agent_goldens.py drives the reference's
``SileroVADAgent`` through and tests/test_vad_agent_cpu.py replays, the scripted detectors, and the trace both record.

A push is (number of samples, probability per whole window).  Its samples are made here: a ramp that goes on from push to push
(so that first and last samples of an output tell which samples it holds), with the first sample of every whole window replaced
by that window's probability - the scripted Silero-style model reads a window's probability off the window itself.
"""
import random
import re

import numpy as np

RATE = 16000
STATE_FIELDS = ("silence_acc_ms", "speech_acc_ms", "source_finished", "is_fresh_state", "consecutive_silence_decay_count")


def push_samples(n, probs, window, start):
    x = (((np.arange(start, start + n) % 1021) + 1) / 2048.0).astype(np.float32)  # exact in fp32, short in JSON
    for w, p in enumerate(probs):
        x[w * window] = np.float32(p)
    return x


class WindowModel:
    """Silero-style: ``model(window, sample_rate) -> tensor`` whose value is the window's first sample; counts its resets."""

    def __init__(self):
        self.resets = 0
        self.calls = 0

    def __call__(self, window, sample_rate):
        assert sample_rate == RATE
        self.calls += 1
        return window[0]

    def reset_states(self):
        self.resets += 1


class ChunkDetector:
    """``speech_probs(chunk)``: the first sample of every whole window.  ``window`` as the stage's."""

    def __init__(self, window=512):
        self.window, self.resets, self.calls = window, 0, 0

    def speech_probs(self, chunk):
        self.calls += 1
        chunk = np.asarray(chunk, dtype=np.float32)
        return [float(chunk[i]) for i in range(0, len(chunk) - self.window + 1, self.window)]

    def reset(self):
        self.resets += 1


# ---- scenarios -------------------------------------------------------------------------------------------------------------
S, Q = 0.9, 0.1  # speech, quiet


def _push(n, probs, lang=None):
    return {"n": int(n), "p": [float(np.float32(p)) for p in probs], "lang": lang}


def _runs(letters):
    """"aaaaaaaaab" -> "a9b": a run of three or more letters as the letter and its length"""
    return re.sub(r"([a-z])\1{2,}", lambda m: f"{m.group(1)}{len(m.group(0))}", letters)


def pack_steps(steps, alphabet):
    """the pushes as [n, one letter per window (its probability's place in ``alphabet``, runs shortened), lang if any]; a reset as 0"""
    out = []
    for s in steps:
        if s.get("reset"):
            out.append(0)
        else:
            out.append([s["n"], _runs("".join(chr(97 + alphabet.index(p)) for p in s["p"]))] + ([s["lang"]] if s["lang"] else []))
    return out


def unpack_steps(packed, alphabet):
    def probs(text):
        return [alphabet[ord(c) - 97] for c, n in re.findall(r"([a-z])(\d*)", text) for _ in range(int(n or 1))]

    return [RESET if s == 0 else {"n": s[0], "p": probs(s[1]), "lang": s[2] if len(s) > 2 else None} for s in packed]


def pack_trace(trace, values):
    """the first and last sample of a written segment (places 12, 13 of its record) as their places in ``values``"""
    return [r[:12] + [values.index(r[12]), values.index(r[13])] + r[14:] if len(r) > 11 else r for r in trace]


def unpack_trace(packed, values):
    return [r[:12] + [values[r[12]], values[r[13]]] + r[14:] if len(r) > 11 else r for r in packed]


def alphabet_of(scns):
    return sorted({p for scn in scns for s in scn["steps"] if not s.get("reset") for p in s["p"]})


def _full(p, chunks=1, n=5120, window=512, lang=None):
    return [_push(n, [p] * (n // window), lang) for _ in range(chunks)]


RESET = {"reset": True}


def hand_written():
    out = []

    def scn(name, steps, **opts):
        out.append({"name": name, "opts": opts, "steps": steps})

    scn("silent_start", _full(Q, 4) + _full(S, 2) + _full(Q, 3))
    scn("fresh_prob_between_0.6_and_0.75", _full(0.7, 2) + _full(0.76, 1) + _full(0.7, 1) + _full(Q, 3))
    scn("fresh_threshold_off", _full(0.7, 2) + _full(Q, 3), init_speech_prob=0.0)
    # the limit inside one chunk: 640 ms of silent windows behind 2 speech windows reach 700 only with what came before
    scn("limit_inside_one_chunk", _full(S, 1) + [_push(5120, [S] + [Q] * 9)] + [_push(12800, [S] * 2 + [Q] * 23)] + _full(Q, 1))
    scn("limit_across_chunks", _full(S, 2) + _full(Q, 3) + _full(S, 1) + _full(Q, 3))
    scn("silence_to_speech_halving", _full(S, 1) + _full(Q, 2) + [_push(5120, [Q] * 6 + [S] * 4)] + _full(Q, 2) + [_push(5120, [Q] * 9 + [S])]
        + _full(Q, 3))
    scn("halving_reaches_the_limit", _full(S, 1) + _full(Q, 2) + [_push(5120 * 3, [Q] * 29 + [S])] + _full(S, 1) + _full(Q, 3))
    scn("three_decays_in_a_row", _full(S, 1) + _full(Q, 2) + _full(S, 5) + _full(Q, 2) + [_push(5120, [S] * 5 + [Q] * 5)] * 5 + _full(Q, 3))
    scn("soft_limit_after_12_s", _full(S, 3, n=64000) + _full(Q, 2) + _full(S, 2) + _full(Q, 3))
    scn("soft_limit_small", _full(S, 4) + _full(Q, 1) + [_push(5120, [S] + [Q] * 9)] + _full(Q, 2), speech_soft_limit_ms=1000)
    scn("no_multiple_of_the_window", [_push(5120 + 200, [S] * 10), _push(700, [S]), _push(511, []), _push(3000, [Q] * 5), _push(5000, [Q] * 9),
                                      _push(5000, [Q] * 9), _push(1234, [S, S])] + _full(Q, 3))
    scn("other_chunk_lengths", [_push(1024, [S, S]), _push(2048, [S] * 4), _push(16000, [S] * 31), _push(8192, [Q] * 16), _push(8192, [Q] * 16),
                                _push(512, [S]), _push(16384, [Q] * 32)])
    scn("shorter_than_one_window", [_push(100, []), _push(511, [])] + _full(S, 1) + [_push(300, [])] * 3 + _full(Q, 2) + [_push(400, [])] + _full(Q, 1))
    scn("speech_after_source_finished_then_reset", _full(S, 2) + _full(Q, 3) + _full(S, 2) + [_push(2000, [S] * 3)] + _full(Q, 1) + [RESET] + _full(S, 1)
        + _full(Q, 3) + [RESET] + _full(Q, 1))
    scn("partial_flush", _full(S, 1) + [_push(3000, [S] * 5)] + _full(Q, 3) + [RESET] + [_push(1000, [S])] + _full(Q, 3))
    scn("other_options", _full(S, 3, n=4000, window=400) + _full(Q, 4, n=4000, window=400) + _full(S, 1, n=4000, window=400),
        window_size_samples=400, chunk_size_samples=3000, silence_limit_ms=500)
    scn("tgt_lang_travels", _full(S, 1, lang="fra") + _full(S, 1, lang="deu") + _full(Q, 3, lang="deu") + [RESET] + _full(S, 1) + _full(Q, 3, lang="spa"))
    scn("reset_in_the_middle", _full(S, 2) + [_push(2000, [S] * 3)] + [RESET] + _full(S, 1) + _full(Q, 1) + [RESET] + _full(Q, 1) + _full(S, 1) + _full(Q, 3))
    scn("threshold_edges", [_push(5120, [0.75] * 10), _push(5120, [0.6] * 10), _push(5120, [0.75001] * 10), _push(5120, [0.6] * 10),
                            _push(5120, [0.60001] * 10)] + _full(0.6, 3))
    return out


def seeded(count=185):
    out = []
    for seed in range(count):
        rng = random.Random(1000 + seed)
        opts = {}
        if seed % 5 == 1:
            opts = {"silence_limit_ms": rng.choice([300, 500, 1000]), "speech_soft_limit_ms": rng.choice([1000, 3000])}
        if seed % 7 == 2:
            opts["chunk_size_samples"] = rng.choice([2048, 4000, 8000])
        if seed % 11 == 3:
            opts["init_speech_prob"] = rng.choice([0.0, 0.3])
        window = 512
        steps, talking = [], False
        for _ in range(rng.randint(3, 4)):  # few and long pushes: the record stays small
            if rng.random() < 0.06:
                steps.append(RESET)
                continue
            n = rng.choice([5120, 5120, 16000, 16000, 8000, 2560, 300, 5120 + rng.randint(1, 600)])
            probs, level = [], rng.choice([0.62, 0.7, 0.8, 0.95]) if talking else rng.choice([0.05, 0.3, 0.55, 0.6])
            for _w in range(n // window):
                if rng.random() < (0.15 if talking else 0.10):  # a level holds until the next change: runs pack well
                    talking = not talking
                    level = rng.choice([0.62, 0.7, 0.8, 0.95]) if talking else rng.choice([0.05, 0.3, 0.55, 0.6])
                probs.append(level)
            steps.append(_push(n, probs, rng.choice([None, None, "fra", "deu"])))
        out.append({"name": f"seed_{seed}", "opts": opts, "steps": steps})
    return out


def scenarios():
    return hand_written() + seeded()


def _num(v):
    """a state value as JSON keeps it shortest: True / False as 1 / 0, a float without a fraction as an int (equal under ==)"""
    if isinstance(v, bool):
        return int(v)
    return int(v) if isinstance(v, float) and v == int(v) else v


# ---- the trace -------------------------------------------------------------------------------------------------------------
def drive(agent, scn, window, SpeechSegment, qsize, resets):
    """Pushes the script through ``agent`` (push + pop per step) -> the record per step.  ``qsize(queue)`` and ``resets()`` hide
    what differs between the reference's class and the restated one."""
    trace, start = [], 0
    for step in scn["steps"]:
        if step.get("reset"):
            agent.reset()
            out = None
        else:
            x = push_samples(step["n"], step["p"], window, start)
            start += step["n"]
            agent.push(SpeechSegment(content=x, sample_rate=RATE, tgt_lang=step["lang"], finished=False))
            out = agent.pop()
        st = agent.states
        rec = [_num(getattr(st, f)) for f in STATE_FIELDS] + [qsize(st.input_queue), qsize(st.next_input_queue), len(st.input_chunk), resets()]
        if out is not None and out.is_empty:  # + empty?, finished
            rec += [1, int(bool(out.finished))]
        elif out is not None:  # + empty?, finished, length, first and last sample, tgt_lang
            rec += [0, int(bool(out.finished)), len(out.content), float(out.content[0]), float(out.content[-1]), out.tgt_lang]
        trace.append(rec)
    return trace
