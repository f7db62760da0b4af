"""Write the fixtures under ``tests/golden/reference/`` from a checkout of the reference project (data files only:
its default config, its recorded result JSONs and a reduced copy of its cached logit-lens pairs).

    python tools/make_golden_fixtures.py <reference root> [tests/golden/reference]

A cached pair ``src/data/processed/<word>/prompt_NN.npz`` holds ``all_probs`` [42, T, 256000] fp32 (1.2 GB in memory)
and the layer-31 residuals.  The tests read layer 31 only, and of that only what decides a response-sum's top-5, so the
fixture keeps per pair:

* ``cols``  -- the vocabulary ids kept: every position's top-16 ids, and the top-64 ids of the sum over all positions
               and of the sum over the response positions (any id left out is below the 16th at every position);
* ``vals``  -- ``all_probs[31][:, cols]`` fp32, exactly as stored;
* ``probs_shape`` / ``resid_shape`` -- the shapes of ``all_probs[31]`` and ``residual_stream_l31``.

The script checks that the reduced pair reproduces the full pair's response-sum top-8 ids and values bit for bit.
"""
import json
import os
import shutil
import sys

import numpy as np

FILES = {
    "configs/default.yaml": "default.yaml",
    "results/ll_topk_ship.json": "ll_topk_ship.json",
    "src/results/logit_lens/seed_42/top5_real/logit_lens_evaluation_results.json":
        "results/logit_lens_evaluation_results.json",
    "src/results copy/logit_lens/seed_42/top5_real/logit_lens_evaluation_results.json":
        "results_copy/logit_lens_evaluation_results.json",
}
LAYER, PER_POS, PER_SUM = 31, 16, 64


def response_start(words):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from taboo_brittleness_amd.interp.prompts import find_model_response_start

    return find_model_response_start(words)


def reduce_pair(npz, meta):
    with np.load(npz, allow_pickle=False) as z:
        probs = np.ascontiguousarray(z["all_probs"][LAYER])
        resid_shape = z["residual_stream_l31"].shape
    start = response_start(meta["input_words"])
    keep = set(np.argsort(-probs, axis=1)[:, :PER_POS].ravel().tolist())
    for s in (probs.sum(0), probs[start:].sum(0)):
        keep |= set(np.argsort(-s)[:PER_SUM].tolist())
    cols = np.array(sorted(keep), np.int32)
    vals = probs[:, cols]
    dense = np.zeros_like(probs)
    dense[:, cols] = vals
    a, b = probs[start:].sum(0), dense[start:].sum(0)
    ia, ib = np.argsort(-a)[:8], np.argsort(-b)[:8]
    assert (ia == ib).all() and (a[ia] == b[ib]).all(), npz
    return {"cols": cols, "vals": vals, "probs_shape": np.array(probs.shape, np.int64),
            "resid_shape": np.array(resid_shape, np.int64)}


def main():
    ref = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join("tests", "golden", "reference")
    for src, dst in FILES.items():
        os.makedirs(os.path.dirname(os.path.join(out, dst)), exist_ok=True)
        shutil.copyfile(os.path.join(ref, src), os.path.join(out, dst))
    base = os.path.join(ref, "src", "data", "processed")
    for word in sorted(os.listdir(base)):
        for f in sorted(os.listdir(os.path.join(base, word))):
            if not f.endswith(".npz"):
                continue
            js = os.path.join(base, word, f[:-4] + ".json")
            meta = json.load(open(js))
            os.makedirs(os.path.join(out, "processed", word), exist_ok=True)
            shutil.copyfile(js, os.path.join(out, "processed", word, f[:-4] + ".json"))
            arrays = reduce_pair(os.path.join(base, word, f), meta)
            dst = os.path.join(out, "processed", word, f)
            np.savez_compressed(dst, **arrays)
            print(dst, arrays["vals"].shape, os.path.getsize(dst))


if __name__ == "__main__":
    main()
