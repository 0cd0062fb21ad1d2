"""Child process of tests/test_prefix_gpu.py: ragged prompts against each row's uniform call on the decoder-step family that
the parent's environment selects (SC_DECODER_GEN1 / SC_DECODER_GEN2 are read once per process).  Prints the family of the
greedy step at 5 rows and OK."""
import sys

import numpy as np
import torch


def main():
    from tests import prefix_common as pc
    from tests.test_lid_gpu import _gen, _same, oracle_lid
    from tests.test_score_gpu import model

    o = oracle_lid()
    cfg, sd, tt, hip = model("v2")
    enc, enc_lens = o["enc"].cuda().contiguous(), o["enc_lens"].tolist()
    head = tt.target_prefix(pc.LANG)
    free = _gen(hip, enc, enc_lens, head)
    H = [free[0][b, : free[1][b]].tolist() for b in range(5)]
    prompts = pc.foreign_prompts(H, head, [l - 2 for l in pc.ragged_lens()], cfg.eos_idx)
    for use_graph in (True, False):
        got = _gen(hip, enc, enc_lens, prompts, use_graph=use_graph)
        for b in range(5):
            uni = _gen(hip, enc, enc_lens, prompts[b], use_graph=use_graph)
            assert _same(got, uni, slice(b, b + 1)), (use_graph, b)
            assert got[0][b, : len(prompts[b])].tolist() == prompts[b]
    assert sum(got[0][b, : got[1][b]].tolist() != H[b] for b in range(5)) >= 3
    print("FAMILY", hip.lib.sc_decoder_step_family(hip.handle, 5, 0))
    print("OK")


if __name__ == "__main__":
    torch.cuda.set_device(0)
    np.seterr(all="raise")
    main()
    sys.exit(0)
