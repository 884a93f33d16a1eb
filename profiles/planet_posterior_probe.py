"""hipets.PlaNetPosterior.update against the torch route at conf/dynamics_model/planet.yaml's shape, n_env 1, 4, 16, 64 ->
profiles/planet_posterior.json (or argv[1]).

The torch route is the stand-in's eager modules on the same GPU: at n_env 1 exactly what PlaNetModel.update_posterior runs
(planet.py:592-641), at n_env > 1 the same modules on a batch.  Both routes get the same device-resident uint8 images, actions and
normals.  Rounds take turns (hipets, torch, hipets, ...), each round is REPS updates between two device synchronisations on the host
clock; the medians over the rounds are reported.  Kernel times come from a separate torch.profiler pass over a few updates."""
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "mbrl-lib_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

import hipets  # noqa: E402
import planet_posterior_f64 as pp  # noqa: E402

DEV, REPS, ROUNDS = "cuda:0", 300, 7


def torch_update(model, obs, action, latent, belief, eps):
    """update_posterior's chain of eager launches (planet.py:615-637, :324-333), batched"""
    with torch.no_grad():
        x = obs.float() / 256.0 - 0.5
        nb = model.belief_model.rnn(model.belief_model.embedding_layer(torch.cat([latent, action], dim=1)), belief)
        for layer in model.encoder.convs:
            x = layer(x)
        enc = model.encoder.fc(x.view(x.size(0), -1))
        params = model.posterior_transition_model(torch.cat([nb, enc], dim=1))
        L = model.latent_state_size
        return params[:, :L] + (F.softplus(params[:, L:]) + model.min_std) * eps, nb


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / REPS * 1e6


def kernel_times(fn, n=20):
    """{kernel name: mean microseconds per call} of the device kernels `fn` launches"""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
        if t and ("posterior" in ev.key or "Cijk" in ev.key or "conv" in ev.key.lower() or "gemm" in ev.key.lower()):
            out[ev.key[:96]] = {"calls_per_update": ev.count / n, "us_per_call": t / ev.count}
    return out


def main():
    case = (pp.CONF_IMAGE, pp.CONF_CONVS, None, pp.CONF)
    L, A, Hb, _ = pp.CONF
    result = {"device": torch.cuda.get_device_name(0), "shape": "conf/dynamics_model/planet.yaml", "reps_per_round": REPS, "rounds": ROUNDS, "n_env": {}}
    engine = hipets.get_engine(DEV)
    for n_env in (1, 4, 16, 64):
        model, obs, actions, eps = pp.make_case(case, n_env)
        gpu_model = __import__("copy").deepcopy(model).to(DEV)
        obs_d, act_d, eps_d = obs[0].to(DEV), actions[0].to(DEV), eps[0].to(DEV)
        post = hipets.PlaNetPosterior(model, n_env=n_env, engine=engine)
        post.reset()
        post.update(obs_d, eps=eps_d)
        state = [torch.zeros(n_env, L, device=DEV), torch.zeros(n_env, Hb, device=DEV)]

        def ours():
            post.update(obs_d, action=act_d, eps=eps_d)

        def ours_kernels():  # the library calls alone: no state clones, no argument conversion
            engine.planet_posterior_update(obs_d, post.latent, post.belief, action=act_d, eps=eps_d)

        def theirs():
            state[0], state[1] = torch_update(gpu_model, obs_d, act_d, state[0], state[1], eps_d)

        for fn in (ours, ours_kernels, theirs):  # warm-up of every shape
            for _ in range(20):
                fn()
        rounds = {"hipets_update": [], "hipets_engine_call": [], "torch": []}
        for _ in range(ROUNDS):
            rounds["hipets_update"].append(timed(ours))
            rounds["hipets_engine_call"].append(timed(ours_kernels))
            rounds["torch"].append(timed(theirs))
        spec = post.spec
        entry = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in rounds.items()}
        entry["hipets_launches_per_update"] = len(spec.conv_weights) + (spec.w_fc is not None) + 2
        entry["torch_over_hipets_update"] = entry["torch"]["median_us"] / entry["hipets_update"]["median_us"]
        try:
            entry["hipets_kernels"] = kernel_times(ours_kernels)
            entry["torch_kernels"] = kernel_times(theirs)
        except Exception as exc:  # the profiler is optional: the timings above do not depend on it
            entry["kernels_not_measured"] = repr(exc)
        result["n_env"][str(n_env)] = entry
        print(n_env, json.dumps({k: v for k, v in entry.items() if "kernels" not in k}), flush=True)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "planet_posterior.json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
