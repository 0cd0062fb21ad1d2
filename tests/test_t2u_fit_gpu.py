"""GPU: sc_t2u_nar_fit on the tiny model (n = 3, ragged text lengths) - the contracts of DESIGN.md section 7v:

(a) all targets 0 and hi = f: every output equals sc_t2u_nar(duration_factor = f) - units, lengths, durations;
(b) row b of a fit call equals row b of the uniform call on the same batch with duration_factor = factors[b];
(c) unit_lens[b] <= target[b] unless flag OVER.
Targets are 0.9x and 0.3x of the natural unit count (taken from a t2u_nar call first), so the fitted and the OVER branch both
occur.  A FiLM model is refused without d_cond; refusals name the item."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import common

pytestmark = pytest.mark.gpu
F32 = np.float32
TL = [12, 8, 5]


@functools.lru_cache(maxsize=1)
def _env():
    cfg, sd, vsd, tt, ct = common.tiny_bundle()
    hip = common.make_hip()
    wav, ns = common.pad_waves(common.waves((1.0, 0.8, 1.2)))
    fb, frames = hip.fbank(torch.from_numpy(wav).cuda(), ns)
    enc, enc_lens = hip.encode_speech(fb, frames.tolist())
    text = common.random_text_seqs(cfg, tt, 3, TL, seed=5)
    hidden = hip.decode_text(enc, enc_lens.tolist(), text).contiguous()
    natural = hip.t2u_nar(hidden, text, TL, 1.0)
    return hip, hidden, text, natural


def _same_rows(a_units, a_lens, b_units, b_lens, b):
    assert int(a_lens[b]) == int(b_lens[b])
    assert a_units[b, : a_lens[b]].tolist() == b_units[b, : b_lens[b]].tolist()


def test_without_targets_the_fit_is_the_uniform_call():
    hip, hidden, text, natural = _env()
    for f in (1.0, 0.8, 1.3):
        want = hip.t2u_nar(hidden, text, TL, f)
        got = hip.t2u_nar_fit(hidden, text, TL, [0, 0, 0], 0.5, f)
        for w, g in zip(want, got[:5]):  # units, unit_lens, durations, char ids, char_seq_lens
            assert w.shape == g.shape and w.tolist() == g.tolist()
        assert got[5].tolist() == [F32(f)] * 3 and got[6].tolist() == [0, 0, 0]
    assert hip.t2u_nar(hidden, text, TL, 1.0)[0].tolist() == natural[0].tolist()  # the handle is as it was


def test_rows_equal_the_uniform_call_at_their_own_factor_and_stay_within_the_target():
    hip, hidden, text, natural = _env()
    nat = natural[1]
    targets = [int(0.9 * nat[0]), int(0.3 * nat[1]), 0]
    lo, hi = 0.75, 1.0
    units, ulens, dur, cids, clens, factors, flags = hip.t2u_nar_fit(hidden, text, TL, targets, lo, hi)
    print("natural", nat.tolist(), "targets", targets, "unit_lens", ulens.tolist(), "factors", factors.tolist(), "flags", flags.tolist())
    assert flags.tolist() == [0, 1, 0]  # fitted, OVER, free
    assert F32(lo) < factors[0] < F32(hi) and factors[1] == F32(lo) and factors[2] == F32(hi)
    assert ulens[0] <= targets[0] and ulens[1] > targets[1] and ulens[2] == nat[2]  # (c)
    assert clens.tolist() == natural[4].tolist() and cids.tolist() == natural[3].tolist()
    for b in range(3):  # (b)
        u_units, u_lens, u_dur, _, _ = hip.t2u_nar(hidden, text, TL, float(factors[b]))
        _same_rows(units, ulens, u_units, u_lens, b)
        assert dur[b].tolist() == u_dur[b].tolist()
        assert int(dur[b].sum()) == int(ulens[b]) and not dur[b, clens[b]:].any()
    # the largest grid factor that fits: two grid steps on (at least the next point, whatever the rounding) the target is passed
    step = (F32(hi) - F32(lo)) * F32(2.0 ** -16)
    over = hip.t2u_nar(hidden, text, TL, float(F32(factors[0]) + F32(2) * step))[1]
    assert over[0] > targets[0]


def test_refusals_name_the_item_and_film_needs_cond():
    hip, hidden, text, natural = _env()
    lib = hip.lib
    tl, ts = np.asarray(TL, dtype=np.int32), np.ascontiguousarray(text.astype(np.int32))
    P = lambda a: C.c_void_p(a.ctypes.data)

    def call(target=(5, 5, 5), lo=(0.75, 0.75, 0.75), hi=(1.0, 1.0, 1.0), handle=None, null=None, cond=None):
        t, l, h = np.asarray(target, dtype=np.int32), np.asarray(lo, dtype=F32), np.asarray(hi, dtype=F32)
        ul, f, fl = np.zeros(3, np.int32), np.zeros(3, F32), np.zeros(3, np.int32)
        su, sc = C.c_int32(0), C.c_int32(0)
        args = [handle or hip.handle, C.c_void_p(hidden.data_ptr()), 3, hidden.shape[1], P(tl), P(ts), P(t), P(l), P(h), cond, P(ul), C.byref(su), C.byref(sc),
                P(f), P(fl)]
        if null is not None:
            args[null] = None
        return lib.sc_t2u_nar_fit(*args), lib.sc_last_error().decode()

    before = hip.t2u_nar(hidden, text, TL, 1.0)
    for kw in (dict(target=(5, 5, -2)), dict(lo=(0.75, 0.75, 0.0)), dict(lo=(0.75, 0.75, -0.5)), dict(lo=(0.75, 0.75, 1.25)),
               dict(hi=(1.0, 1.0, float("inf"))), dict(lo=(0.75, 0.75, float("nan")))):
        rc, msg = call(**kw)
        assert rc == -1 and "item 2" in msg, (kw, msg)
    for null in (0, 1, 4, 5, 6, 7, 8, 13, 14):
        rc, msg = call(null=null)
        assert rc == -1 and "null" in msg, (null, msg)
    # a model without FiLM takes no conditioning vectors
    cond = torch.zeros(3, 8, device="cuda")
    rc, msg = call(cond=C.c_void_p(cond.data_ptr()))
    assert rc == -1 and "FiLM" in msg
    assert hip.t2u_nar(hidden, text, TL, 1.0)[0].tolist() == before[0].tolist()  # refusals leave the handle usable


def test_a_film_model_is_refused_without_cond_and_fits_with_it():
    from seamless_communication_amd import cards, synthetic as syn
    from seamless_communication_amd.config import tiny_expressive_config
    from seamless_communication_amd.runtime import HipS2STModel, SeamlessHipError
    from seamless_communication_amd.tokenizer import CharTokenizer, NllbTextTokenizer
    from tests import expressive_oracle as eo

    cfg = tiny_expressive_config()
    tt = NllbTextTokenizer(cfg.text_vocab_size, cards.TEXT_LANGS)
    hip = HipS2STModel(cfg, syn.make_unity_state_dict(cfg, eo.T2U_SEED), None, device=0)
    hip.set_nar_tables(tt, CharTokenizer(cfg.char_vocab_size))
    wav, ns = common.pad_waves(common.waves((1.0, 0.8, 0.6)))
    fb, frames = hip.fbank(torch.from_numpy(wav).cuda(), ns)
    enc, enc_lens = hip.encode_speech(fb, frames.tolist())
    tl = list(eo.T2U_TEXT_LENS)
    text = common.random_text_seqs(cfg, tt, 3, tl, seed=eo.T2U_TEXT_SEED)
    dec = hip.decode_text(enc, enc_lens.tolist(), text).contiguous()
    cond = eo.cond_rows(3, cfg.film_cond_dim).cuda()
    with pytest.raises(SeamlessHipError, match="FiLM"):
        hip.t2u_nar_fit(dec, text, tl, [0, 0, 0], 0.75, 1.0)
    want = hip.t2u_nar(dec, text, tl, 0.9, cond=cond)
    got = hip.t2u_nar_fit(dec, text, tl, [0, 0, 0], 0.75, 0.9, cond=cond)
    for w, g in zip(want, got[:5]):
        assert w.tolist() == g.tolist()
    targets = [int(0.9 * want[1][0]), 0, int(0.9 * want[1][2])]
    units, ulens, dur, _, _, factors, flags = hip.t2u_nar_fit(dec, text, tl, targets, 0.5, 0.9, cond=cond)
    for b in range(3):
        u_units, u_lens, u_dur, _, _ = hip.t2u_nar(dec, text, tl, float(factors[b]), cond=cond)
        _same_rows(units, ulens, u_units, u_lens, b)
        assert dur[b].tolist() == u_dur[b].tolist() and (ulens[b] <= targets[b] or targets[b] == 0 or flags[b] == 1)
