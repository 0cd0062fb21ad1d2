"""GPU: what the text-generation C entries refuse, the words they refuse it with and the order of their checks - one table,
called through ``hip.lib`` as tests/test_cabi_cpu.py calls the library.  The tiny model of the neighbouring tests, n = 2,
s_enc = 4, a two-token prompt.  Every row is refused on the host before any launch with the invalid-argument status, and after
each refusal a valid generate_text call on the same handle returns the ids it returned before: a refusal leaves no half-built
session behind.

Two refusals of the same family are asserted elsewhere with the same input and are not repeated here:
sc_generate_text_nbest with nbest = beam_size + 1 (tests/test_nbest_gpu.py: test_refusals_name_their_reason_and_leave_the_handle_usable)
and sc_generate_text_capture with beam_size = 2 (tests/test_transcriber_gpu.py: test_unsupported_capture_calls_fail_clearly)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import common

pytestmark = pytest.mark.gpu

N, S_ENC, CAP = 2, 4, 12
SC_ERR_INVALID = -1


@functools.lru_cache(maxsize=1)
def _env():
    hip = common.make_hip()
    cfg, _, _, tt, _ = common.tiny_bundle()
    enc = torch.randn(N, S_ENC, cfg.model_dim, generator=torch.Generator().manual_seed(11)).cuda().contiguous()
    prompt = np.asarray(tt.target_prefix("fra"), dtype=np.int32)
    assert len(prompt) == 2
    want = _valid(hip, enc, prompt)
    return hip, cfg, enc, prompt, want


def _valid(hip, enc, prompt):
    ids, lens, scores, _ = hip.generate_text(enc, [S_ENC] * N, prompt.tolist(), hard_max_seq_len=CAP, want_hidden=False)
    return ids.copy()


class Call:
    """The arguments of one valid call of every entry; a case replaces one of them (two for the row that pins an order)."""

    def __init__(self, hip, cfg, enc, prompt):
        from seamless_communication_amd import _lib

        self.hip, self.enc = hip, enc
        self.n, self.s_enc = N, S_ENC
        self.el = np.full(N, S_ENC, dtype=np.int32)
        self.opts = hip._gen_opts(1, (1, 200), CAP, 1, 0.0, True)
        self.prefix = prompt.copy()
        self.rows = np.ascontiguousarray(np.tile(prompt, (N, 1)))
        self.plens = np.full(N, 2, dtype=np.int32)
        self.ids, self.lens, self.scores = np.zeros((N, CAP), np.int32), np.zeros(N, np.int32), np.zeros(N, np.float32)
        self.step = np.zeros((N, CAP), np.float32)
        self.hidden = torch.zeros(N, CAP - 1, cfg.model_dim, device="cuda")
        self.xattn = torch.zeros(N, CAP, S_ENC, device="cuda")
        self.b_tok, self.b_off, self.n_banned = None, None, 0
        self.p_tok, self.p_off, self.n_boost, self.boost = None, None, 0, 0.0
        self.sopts = _lib.sc_sample_opts()
        self.sopts.abi_version, self.sopts.num_gens, self.sopts.top_k = _lib.SC_ABI_VERSION, 1, 0
        self.sopts.top_p, self.sopts.temperature, self.sopts.seed = 1.0, 1.0, 0
        self.tokens = np.ascontiguousarray(np.tile(np.asarray([prompt[0], prompt[1], 7], dtype=np.int32), (N, 1)))

    def run(self, entry):
        from seamless_communication_amd.runtime import _ptr

        s, lib, h = self, self.hip.lib, self.hip.handle
        src = (h, _ptr(s.enc), s.n, s.s_enc, _ptr(s.el))
        out = (_ptr(s.ids), _ptr(s.lens), _ptr(s.scores), _ptr(s.hidden))
        banned = (_ptr(s.b_tok), _ptr(s.b_off), s.n_banned)
        boost = (_ptr(s.p_tok), _ptr(s.p_off), s.n_boost, float(s.boost))
        one = (C.byref(s.opts), _ptr(s.prefix), len(s.prefix))
        if entry == "sc_generate_text":
            return lib.sc_generate_text(*src, *one, *out)
        if entry == "sc_generate_text_banned":
            return lib.sc_generate_text_banned(*src, *one, *out, *banned)
        if entry == "sc_generate_text_boosted":
            return lib.sc_generate_text_boosted(*src, *one, *out, *banned, *boost)
        if entry == "sc_generate_text_rows":
            return lib.sc_generate_text_rows(*src, C.byref(s.opts), _ptr(s.rows), s.rows.shape[1], *out)
        if entry == "sc_generate_text_prompts":
            return lib.sc_generate_text_prompts(*src, C.byref(s.opts), _ptr(s.rows), s.rows.shape[1], _ptr(s.plens), *out, *banned, *boost)
        if entry == "sc_generate_text_sampled":
            return lib.sc_generate_text_sampled(*src, C.byref(s.opts), C.byref(s.sopts), _ptr(None), _ptr(s.prefix), len(s.prefix), _ptr(s.ids),
                                                _ptr(s.lens), _ptr(s.scores), _ptr(s.step), _ptr(None), *banned)
        if entry == "sc_generate_text_capture":
            return lib.sc_generate_text_capture(*src, *one, _ptr(s.ids), _ptr(s.lens), _ptr(s.scores), _ptr(None), _ptr(s.xattn), _ptr(s.step))
        if entry == "sc_decode_text":
            return lib.sc_decode_text(*src, _ptr(s.tokens), s.tokens.shape[1], _ptr(s.hidden))
        raise AssertionError(entry)


def _banned_minus_one(c, cfg):
    c.n_banned = -1


def _boost_null(c, cfg):
    c.n_boost = 1


def _boost_not_finite(c, cfg):
    c.p_tok, c.p_off, c.n_boost, c.boost = np.asarray([5], np.int32), np.asarray([0, 1], np.int32), 1, float("inf")


def _row_token_is_vocab_size(c, cfg):
    c.rows[1, 1] = cfg.text_vocab_size


def _row_of_length_zero(c, cfg):
    c.plens[1] = 0


def _banned_minus_one_and_row_of_length_zero(c, cfg):
    c.n_banned = -1
    c.plens[1] = 0


def _other_abi_version(c, cfg):
    c.sopts.abi_version += 1


def _null_xattn(c, cfg):
    c.xattn = None


def _enc_len_past_s_enc(c, cfg):
    c.el[1] = S_ENC + 1


def _min_seq_len_above_max(c, cfg):
    c.opts.min_seq_len = CAP + 1


def _no_rows(c, cfg):
    c.n = 0


# (entry, the bad input, what sc_last_error must contain)
TABLE = [
    ("sc_generate_text_banned", _banned_minus_one, "sc_generate_text_banned: bad banned list"),
    ("sc_generate_text_boosted", _boost_null, "sc_generate_text_boosted: bad phrase list"),
    ("sc_generate_text_boosted", _boost_not_finite, "boost phrases: boost must be finite with |boost| <= "),
    ("sc_generate_text_rows", _row_token_is_vocab_size, "sc_generate_text_rows: prompt token"),
    ("sc_generate_text_prompts", _row_of_length_zero, "prompt length 0 outside 1.."),
    ("sc_generate_text_prompts", _banned_minus_one_and_row_of_length_zero, "sc_generate_text_prompts: bad banned list"),
    ("sc_generate_text_sampled", _other_abi_version, "options ABI version"),
    ("sc_generate_text_capture", _null_xattn, "null argument"),
    ("sc_generate_text", _enc_len_past_s_enc, "out of range"),
    ("sc_generate_text", _min_seq_len_above_max, "min_seq_len"),
    ("sc_decode_text", _no_rows, "sc_generate_text: empty batch"),
]


@pytest.mark.parametrize("entry,spoil,words", TABLE, ids=[f"{e}-{f.__name__.lstrip('_')}" for e, f, _ in TABLE])
def test_refusal_names_its_reason_and_leaves_the_handle_usable(entry, spoil, words):
    hip, cfg, enc, prompt, want = _env()
    call = Call(hip, cfg, enc, prompt)
    spoil(call, cfg)
    hip._after_torch()
    status = call.run(entry)
    message = hip.lib.sc_last_error().decode()
    assert status == SC_ERR_INVALID, (status, message)
    assert words in message, message
    assert np.array_equal(_valid(hip, enc, prompt), want)


def test_every_entry_of_the_table_takes_its_unspoilt_call():
    """The arguments a case starts from are valid for every entry: a refusal above is the spoilt input's doing."""
    hip, cfg, enc, prompt, want = _env()
    for entry in sorted({e for e, _, _ in TABLE}):
        call = Call(hip, cfg, enc, prompt)
        hip._after_torch()
        assert call.run(entry) == 0, (entry, hip.lib.sc_last_error().decode())
        if entry not in ("sc_decode_text", "sc_generate_text_sampled"):
            assert np.array_equal(call.ids, want), entry
