"""Records tests/golden/replay_buffer_cases.npz on the CPU from the reference's own mbrl.util.ReplayBuffer and
mbrl.algorithms.mbpo.maybe_replace_sac_buffer (needs the reference checkout; run by hand: `python tests/make_replay_golden.py`).
The scripted sequence is replay_restatement.run_script: capacity 37, obs 3, act 2, default_rng(5); add_batch of 10, 20, 15 (wraps) and
37 rows (an exact lap), add, sample(8) twice, get_all(shuffle=True), save / load, a growth to 50 and a shrink to 30.  After every
operation: the stored rows, cur_idx, num_stored, the sampled batches and the generator's state (as JSON)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import replay_restatement as rr  # noqa: E402
from oracle import ref_bridge  # noqa: E402

OUT = os.path.join(HERE, "golden", "replay_buffer_cases.npz")


def main():
    import types

    ref_bridge.import_reference()
    sys.modules.setdefault("imageio", types.ModuleType("imageio"))  # (mbpo.py imports a video recorder this run never touches)
    import mbrl.util
    from mbrl.algorithms.mbpo import maybe_replace_sac_buffer

    rec, _ = rr.run_script(mbrl.util.ReplayBuffer, maybe_replace_sac_buffer)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT}: {len(rec)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
