#!/usr/bin/env python
"""Generate tests/golden/reference_fuzz.json: digests (oracle/ref_harness.py: fuzz_digests) of what the REAL reference's tokenizers
and row parser return on the seeded corpora the tests build (their fuzz_texts() / parse_row_cases() / wordpiece_texts()), so that the
tests compare against the reference without a reference checkout.  Re-run where the reference is importable:

    python tools/make_golden_fuzz.py
"""
from __future__ import annotations

import gzip
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_harness as R  # noqa: E402


def entry(pairs, table=None):
    e = {"chunks": R.fuzz_digests(pairs)}
    if table is not None:
        e["table"] = R.digest(sorted(table.items()))
    return e


def main(d):
    R.install_shims()
    import test_bpe_tokenizer as TB
    import test_dataset as TD
    import test_wukong_data as TW
    from easynlp.appzoo.wukong_clip.bert_tokenizer import FullTokenizer
    from easynlp.modelzoo import BertTokenizer
    from easynlp.modelzoo.models.clip.openclip_tokenizer import SimpleTokenizer
    from easynlp.utils import parse_row_by_schema
    out = {}
    bpe = os.path.join(d, "bpe.txt.gz")
    with gzip.open(bpe, "wb") as f:
        f.write(np.load(TB.GOLD)["merges"].tobytes())
    ref = SimpleTokenizer(bpe_path=bpe)
    out["openclip_bpe"] = entry([[t, ref.encode(t)] for t in TB.fuzz_texts()], ref.encoder)
    vocab = os.path.join(d, "vocab.txt")
    with open(vocab, "wb") as f:
        f.write(np.load(TW.GOLD)["vocab"].tobytes() + b"\n")      # (the same BERT-layout vocabulary serves the word-piece loader)
    ref = FullTokenizer(vocab_file=vocab)
    out["wukong_tokenizer"] = entry([[t, ref.tokenize(t)] for t in TW.fuzz_texts()], ref.vocab)
    out["parse_row"] = entry([[c, parse_row_by_schema(*c)] for c in TD.parse_row_cases()])
    ref = BertTokenizer.from_pretrained(vocab)
    out["wordpiece"] = entry([[t, TD.wordpiece_encode(ref, t)] for t in TD.wordpiece_texts()])
    with open(R.FUZZ_DIGESTS, "w", encoding="utf-8") as f:       # one line per corpus
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in out.items()) + "\n}\n")
    print("wrote", R.FUZZ_DIGESTS)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        main(d)
