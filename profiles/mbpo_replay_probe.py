"""MBPO's SAC replay buffer on the device against on the host, at the mbpo_halfcheetah shape (100 000 rollout rows, obs 17, act 6,
policy 17-512-512, batch 256): what a hipets.DeviceReplayBuffer changes in hipets.rollout_model_and_populate_sac_buffer and in
SACUpdater.update_many.  The comparison route is the host-buffer path of the same two functions.

    python profiles/mbpo_replay_probe.py [--out profiles/mbpo_replay.json] [--rows 100000] [--reps 20] [--host-only]

--host-only measures the host-buffer route alone (it runs on a commit without the device buffer too: the parent's numbers).
Protocol of profiles/mbpo_populate_probe.py: a host clock around calls that end in a synchronisation, 3 warm-up calls, the median of
--reps with min and p90; device events around single launches, in windows of their own.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mbrl-lib_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")):
    if p not in sys.path:
        sys.path.insert(0, p)

import hipets  # noqa: E402
import mbpo_populate_probe as pp  # noqa: E402
import sac_restatement as sr  # noqa: E402
from sac_update_probe import ReplayBuffer as HostSamples  # noqa: E402

OBS, ACT, HID, B, N_UPDATES = 17, 6, 512, 256, 20


def fill(buf, rows, obs, act, seed=2):
    """``rows`` random transitions into a buffer with add_batch (either kind), in chunks of at most its capacity"""
    g = np.random.default_rng(seed)
    done = 0
    while done < rows:
        n = min(rows - done, 100_000, buf.capacity)
        buf.add_batch((g.standard_normal((n, obs)) * 0.5).astype(np.float32), g.uniform(-1, 1, (n, act)).astype(np.float32),
                      (g.standard_normal((n, obs)) * 0.5).astype(np.float32), g.standard_normal(n).astype(np.float32), g.random(n) < 0.05,
                      np.zeros(n, dtype=bool))
        done += n
    return buf


class HostBuffer(pp.Buffer):
    """pp.Buffer with mbrl.util.ReplayBuffer's full sample (six fancy-indexed arrays), what update_many reads"""

    def sample(self, batch_size):
        idx = self.rng.choice(self.stored, size=batch_size)
        tup = (self.obs[idx], self.action[idx], self.next_obs[idx], self.reward[idx], self.terminated[idx], self.truncated[idx])

        class Batch:
            def astuple(self):
                return tup

        return Batch()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mbpo_replay.json"))
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU: no GPU, no numbers"
    dev = torch.device("cuda:0")
    N, reps = args.rows, args.reps
    torch.manual_seed(0)
    engine = hipets.get_engine(dev)
    env = hipets.ModelEnv(pp.synthetic_spec(dev), engine=engine, seed=1)
    sac = sr.TinySAC(OBS, ACT, HID, device=dev)
    up = hipets.SACUpdater(sac, engine=engine)
    agent = pp.TorchAgent(sac.policy, dev)
    rng = np.random.default_rng(0)
    source = pp.Buffer(N, OBS, ACT, rng)
    o = (rng.standard_normal((N, OBS)) * 0.1).astype(np.float32)
    source.add_batch(o, np.zeros((N, ACT), np.float32), o, np.zeros(N, np.float32), np.zeros(N, bool), np.zeros(N, bool))
    res = {"shape": {"rows": N, "obs": OBS, "act": ACT, "policy_hidden": HID, "batch": B, "updates": N_UPDATES},
           "device": torch.cuda.get_device_name(0), "reps": reps, "host_only": bool(args.host_only), "populate": {}}
    routes = ["host"] if args.host_only else ["host", "device"]

    def sac_buffer(route, capacity):
        if route == "host":
            return HostBuffer(capacity, OBS, ACT, np.random.default_rng(3))
        return hipets.DeviceReplayBuffer(capacity, (OBS,), (ACT,), rng=np.random.default_rng(3), engine=engine)

    # ---- the populate, L = 1 and L = 5 (the buffer wraps every other call) ----
    for L in (1, 5):
        res["populate"][f"L{L}"] = {}
        for route in routes:
            sink = sac_buffer(route, 2 * N * L)
            res["populate"][f"L{L}"][route] = pp.wall(lambda: hipets.rollout_model_and_populate_sac_buffer(env, source, agent, sink, True, L, N), reps)
            del sink
    env._return_as_np = True
    # ---- 20 updates, and one iteration: a populate at L = 1 plus 20 updates ----
    count = [0]
    res["update_many_20"], res["iteration_populate_L1_plus_20_updates"] = {}, {}
    for route in routes:
        sink = fill(sac_buffer(route, 2 * N), N, OBS, ACT)

        def updates():
            up.update_many([sink] * N_UPDATES, B, count[0], None, reverse_mask=True)
            count[0] += N_UPDATES

        def iteration():
            hipets.rollout_model_and_populate_sac_buffer(env, source, agent, sink, True, 1, N)
            updates()

        res["update_many_20"][route] = pp.wall(updates, reps)
        res["iteration_populate_L1_plus_20_updates"][route] = pp.wall(iteration, reps)
        del sink
    env._return_as_np = True
    # (the generator's draws of a seeded run: the route sac_update_probe.py measured, for reference against its JSON)
    samples = HostSamples(100_000, OBS, ACT, np.random.default_rng(0))

    def updates_parent_probe():
        up.update_many([samples] * N_UPDATES, B, count[0], None, reverse_mask=True)
        count[0] += N_UPDATES

    res["update_many_20"]["host_as_in_sac_update_probe"] = pp.wall(updates_parent_probe, reps)
    if not args.host_only:
        # ---- the gather launch alone, 20 x 256 rows ----
        res["gather_launch_20x256"] = {}
        for name, (od, ad) in {"obs17_act6": (17, 6), "obs376_act17": (376, 17)}.items():
            buf = fill(hipets.DeviceReplayBuffer(100_000, (od,), (ad,), rng=np.random.default_rng(4), engine=engine), 100_000, od, ad)
            idx = torch.from_numpy(np.random.default_rng(5).integers(0, 100_000, size=N_UPDATES * B)).to(dev)
            out = torch.empty(N_UPDATES * B, buf.width, device=dev)
            s = pp.events(lambda: buf.gather(idx, True, out=out), reps)
            s["bytes_moved"] = 2 * 4 * N_UPDATES * B * buf.width + 8 * N_UPDATES * B
            s["gb_per_s"] = s["bytes_moved"] / (s["median_ms"] * 1e-3) / 1e9
            res["gather_launch_20x256"][name] = s
            # the host's share the gather replaces: 20 x (sample + pack) and the pinned upload
            host = fill(HostBuffer(100_000, od, ad, np.random.default_rng(4)), 100_000, od, ad)
            slab = torch.empty(N_UPDATES, B, buf.width, pin_memory=True)
            res["gather_launch_20x256"][name + "_host_sample_pack_upload"] = pp.wall(
                lambda: ([hipets.mbpo.pack_sac_batch(host.sample(B).astuple(), True, out=slab[i].numpy()) for i in range(N_UPDATES)],
                         slab.to(dev, non_blocking=True)), reps)
            del buf, host
        # ---- one compaction step: into the ring against into the staging area ----
        obs = torch.from_numpy(source.obs).to(dev)
        actor = hipets.SACActor(sac.policy, engine=engine)
        action = actor.act_device(obs, sample=True)
        state = env.reset(source.obs, return_as_np=False)
        nobs, rew, done, _ = env.step(action, state, sample=True)
        env._return_as_np = True
        width = 2 * OBS + ACT + 2
        staging = torch.empty(N * width, device=dev)
        offset, count32 = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        accum = torch.zeros(N, dtype=torch.uint8, device=dev)
        ring = hipets.DeviceReplayBuffer(N + N // 2, (OBS,), (ACT,), engine=engine)  # (wraps in two calls of three)

        def staged():
            offset.zero_()
            accum.zero_()
            engine.compact_transitions(obs, action, nobs, rew.reshape(-1), done.reshape(-1), accum, staging, N, offset, count32)

        def ringed():
            offset.zero_()
            accum.zero_()
            engine.ring_compact_transitions(obs, action, nobs, rew.reshape(-1), done.reshape(-1), accum, ring.storage, ring.capacity, ring.cursor, count32)

        res["compaction_step_with_two_resets"] = {"staging": pp.events(staged, reps), "ring": pp.events(ringed, reps)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    print("\n| what | route | median ms | min | p90 |\n|---|---|---|---|---|")
    rows = [(f"populate L={L}", r, s) for L in (1, 5) for r, s in res["populate"][f"L{L}"].items()]
    rows += [("update_many, 20 updates", r, s) for r, s in res["update_many_20"].items()]
    rows += [("iteration: populate L=1 + 20 updates", r, s) for r, s in res["iteration_populate_L1_plus_20_updates"].items()]
    rows += [("gather launch 20 x 256", r, s) for r, s in res.get("gather_launch_20x256", {}).items()]
    rows += [("compaction step (+ 2 resets)", r, s) for r, s in res.get("compaction_step_with_two_resets", {}).items()]
    for what, route, s in rows:
        print(f"| {what} | {route} | {s['median_ms']:.3f} | {s['min_ms']:.3f} | {s['p90_ms']:.3f} |")


if __name__ == "__main__":
    main()
