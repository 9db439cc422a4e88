"""Writes tests/golden/zstd_dec_blocks/corrupt_sample.json: the sample of the block route's corruption sweep
(tests/zstdd_blocks_mutate.py, gpu_sample) that tests/test_gpu_zstd_dec_blocks_corrupt.py sends to the GPU.  The sweep runs
on the emulator and needs libzstd for rule 3; tests/test_sim_zstdd_blocks_corrupt.py holds the file against the sweep.

    python tests/golden/gen_zstd_dec_blocks_corrupt.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zstdd_blocks_mutate as X
import zstdd_blocks_sim as B

if __name__ == "__main__":
    sweep = X.run(progress=True)
    assert sweep["with_lib"] and not sweep["violations"], sweep["violations"][:20]
    lines = X.gpu_sample(sweep)
    with open(os.path.join(B.GOLDEN, "corrupt_sample.json"), "w") as f:
        json.dump({"what": "base|pos|value|count|status|in_used|out_len|sha256 of an accepted output or -; the line behind a "
                           "mutant's own has the base's count (tests/zstdd_blocks_mutate.py, gpu_sample)",
                   "mutants": sweep["total"], "sample": lines}, f, indent=0)
        f.write("\n")
    print("%d mutants in %.0f s, %d lines" % (sweep["total"], sweep["seconds"], len(lines)))
