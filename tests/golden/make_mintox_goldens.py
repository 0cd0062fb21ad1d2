"""Mints tests/golden/mintox_ref.json from the reference's EXECUTED code: its toxicity/etox_bad_word_checker.py and
toxicity/mintox.py are imported by file path (their fairseq2 / model imports replaced by the placeholder modules below)
and ``ETOXBadWordChecker._preprocess`` / ``get_bad_words`` (plain and sentence-piece path, with the toy
``encode_as_tokens`` below) / ``extract_bad_words``, ``_extract_bad_words_with_batch_indices`` and
``_replace_with_new_text_output_in_batch`` run on seeded cases built from made-up, harmless words.  The JSON holds the
word lists, the inputs and the outputs; tests/test_mintox_cpu.py reads only the JSON.

    python tests/golden/make_mintox_goldens.py <reference>/src/seamless_communication
"""
from __future__ import annotations

import importlib.util
import json
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
OUT = HERE / "mintox_ref.json"

_PLACEHOLDERS = {
    "fairseq2": [],
    "fairseq2.assets": ["AssetCard", "AssetDownloadManager", "AssetStore", "asset_store", "download_manager"],
    "fairseq2.data": ["StringLike", "SequenceData"],
    "fairseq2.data.text": ["SentencePieceEncoder", "SentencePieceModel"],
    "fairseq2.data.text.text_tokenizer": ["TextTokenizer"],
    "fairseq2.data.typing": ["StringLike"],
    "fairseq2.generation": ["BannedSequenceProcessor"],
    "fairseq2.nn": [],
    "fairseq2.nn.padding": ["get_seqs_and_padding_mask"],
    "fairseq2.typing": ["Device"],
    "seamless_communication": [],
    "seamless_communication.inference": ["SequenceGeneratorOptions"],
    "seamless_communication.models": [],
    "seamless_communication.models.unity": ["UnitTokenizer", "UnitYModel"],
    "seamless_communication.toxicity": [],
}


def install_placeholders() -> None:
    """Modules that only have to exist for the two files to import; nothing minted here calls into them."""
    for name, attrs in _PLACEHOLDERS.items():
        if name in sys.modules:
            continue
        mod = types.ModuleType(name)
        mod.__path__ = []
        for a in attrs:
            setattr(mod, a, type(a, (), {}))
        sys.modules[name] = mod


def load(ref_root: Path, rel: str, as_name: str):
    spec = importlib.util.spec_from_file_location(as_name, ref_root / rel)
    m = importlib.util.module_from_spec(spec)
    sys.modules[as_name] = m
    spec.loader.exec_module(m)
    return m


class ToyPieces:
    """``encode_as_tokens``: every space-delimited word in chunks of two characters, the first with a "▁" in front."""

    @staticmethod
    def encode_as_tokens(text):
        out = []
        for w in text.split():
            w = "▁" + w
            out += [w[i: i + 2] for i in range(0, len(w), 2)]
        return out


WORDS = {
    "eng": ["blorf", "snark", "wug fip", "quux"],
    "fra": ["zibble", "blorf"],
    "xyz_Abcd": ["mimsy", "tove"],  # a language + script variant, matched on pieces
    "pqr": ["brillig", "gyre", "mome rath"],  # matched on pieces
}
SP_LANGS = ["xyz_Abcd", "pqr"]
FILLER = ["the", "a", "cat", "sat", "on", "mat", "blorfs", "snarky", "xquux", "wug", "fip", "Hello", "tovex", "gy", "re",
          "mome", "rath", "zib", "ble"]
PUNCT = [",", ".", "!", "?", "-", "+", "'", "(", ")", "*", "_", "★"]


def sentence(rng, lang_words, p_word):
    n = int(rng.integers(0, 9))
    toks = []
    for _ in range(n):
        r = rng.random()
        if r < p_word:
            w = lang_words[int(rng.integers(0, len(lang_words)))]
            w = [w, w.upper(), w.capitalize()][int(rng.integers(0, 3))]
        else:
            w = FILLER[int(rng.integers(0, len(FILLER)))]
        if rng.random() < 0.3:
            w = w + PUNCT[int(rng.integers(0, len(PUNCT)))]
        if rng.random() < 0.15:
            w = PUNCT[int(rng.integers(0, len(PUNCT)))] + w
        toks.append(w)
    return " ".join(toks)


def main():
    ref_root = Path(sys.argv[1])
    install_placeholders()
    etox = load(ref_root, "toxicity/etox_bad_word_checker.py", "seamless_communication.toxicity.etox_bad_word_checker")
    mintox = load(ref_root, "toxicity/mintox.py", "ref_mintox")
    variants = {lang: {w: [w.lower(), w.upper(), w.capitalize()] for w in ws} for lang, ws in WORDS.items()}
    checker = etox.ETOXBadWordChecker(WORDS, variants, ToyPieces(), set(SP_LANGS))
    rng = np.random.default_rng(20241016)
    gold = {"words": WORDS, "sp_langs": SP_LANGS}

    texts = ["", "Hello, World!", "a+b  c_d\te\nf", "ÄÖ ü—ß ★x", "wug  fip", "WUG FIP!", "wug, fip"]
    texts += [sentence(rng, WORDS["eng"], 0.3) for _ in range(12)]
    gold["preprocess"] = [{"text": t, "out": checker._preprocess(t)} for t in texts]

    gold["get_bad_words"] = []
    for lang in WORDS:
        for _ in range(12):
            t = sentence(rng, WORDS[lang], 0.35)
            gold["get_bad_words"].append({"text": t, "lang": lang, "out": checker.get_bad_words(t, lang)})
    try:
        checker.get_bad_words("a", "nope")
        err = None
    except Exception as e:  # noqa: BLE001
        err = [type(e).__name__, str(e)]
    gold["get_bad_words_unknown_lang"] = err

    langs = list(WORDS)
    gold["extract_bad_words"] = []
    for _ in range(32):
        sl, tl = langs[int(rng.integers(0, 4))], langs[int(rng.integers(0, 4))]
        s, t = sentence(rng, WORDS[sl], 0.08), sentence(rng, WORDS[tl], 0.3)
        gold["extract_bad_words"].append({"src": s, "tgt": t, "src_lang": sl, "tgt_lang": tl,
                                          "out": checker.extract_bad_words(s, t, sl, tl)})

    gold["batch"] = []
    for _ in range(12):
        n = int(rng.integers(1, 6))
        sl, tl = langs[int(rng.integers(0, 4))], langs[int(rng.integers(0, 4))]
        src = [sentence(rng, WORDS[sl], 0.05) for _ in range(n)]
        tgt = [sentence(rng, WORDS[tl], 0.25) for _ in range(n)]
        words, rows = mintox._extract_bad_words_with_batch_indices(src, tgt, sl, tl, checker)
        new = [f"new {k}" for k in range(len(rows))]
        replaced = list(tgt)
        mintox._replace_with_new_text_output_in_batch(replaced, rows, new)
        gold["batch"].append({"src": src, "tgt": tgt, "src_lang": sl, "tgt_lang": tl, "words": words, "rows": rows,
                              "new_texts": new, "replaced": replaced})

    OUT.write_text(json.dumps(gold, indent=1, ensure_ascii=False) + "\n")
    n_cases = sum(len(gold[k]) for k in ("preprocess", "get_bad_words", "extract_bad_words", "batch"))
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {n_cases} cases)")


if __name__ == "__main__":
    main()
