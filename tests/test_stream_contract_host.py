"""The coverage table of the stream contract (tests/stream_cases.py), checked without a GPU: every symbol of the ABI that takes a stream
belongs to exactly one class, every symbol that takes part in the ordering is exercised on both sides of a stream switch, and the
chains tests/test_gpu_streams.py runs are this table's."""
import os
import re

import stream_cases as sc
from conftest import ROOT
from hipets import _lib

STREAM_SYMBOLS = sc.stream_symbols(_lib.SYMBOLS)
CLASSES = {"ordered": tuple(sc.ORDERED), "synchronising": sc.SYNCHRONISING, "launch_only": sc.LAUNCH_ONLY, "needs_communicator": sc.NEEDS_COMMUNICATOR}


def test_the_four_classes_partition_the_stream_taking_symbols():
    """a new entry point with a stream parameter fails here until it is given a class"""
    assert len(STREAM_SYMBOLS) == len(set(STREAM_SYMBOLS)) > 40
    listed = [s for members in CLASSES.values() for s in members]
    assert len(listed) == len(set(listed)), f"in two classes: {sorted(s for s in set(listed) if listed.count(s) > 1)}"
    assert set(listed) == set(STREAM_SYMBOLS), (f"without a class: {sorted(set(STREAM_SYMBOLS) - set(listed))}; "
                                               f"no stream-taking symbol of the ABI: {sorted(set(listed) - set(STREAM_SYMBOLS))}")
    # a symbol without a stream parameter cannot take part at all
    assert not [s for s in listed if s not in _lib.SYMBOLS]


def test_every_ordered_symbol_produces_and_consumes_across_a_stream_switch():
    for symbol, where in sc.ORDERED.items():
        assert where["producer"], f"{symbol} is never the producer before a stream switch"
        assert where["consumer"], f"{symbol} is never the consumer after a stream switch"
        assert set(where["producer"]) | set(where["consumer"]) <= set(sc.CHAINS)
    for name, steps in sc.CHAINS.items():
        assert len(steps) >= 2 and len(set(steps)) == len(steps), name
        # the pinned staging ring has four slots: a fifth host observation would block the host behind the gate
        staged = [s for s in steps if re.fullmatch(r"hipets_(rollout|plan_(cem|mppi|icem)(_batched)?)", sc.symbol_of(s))]
        assert len(staged) <= 4, f"{name} stages {len(staged)} host observations"
    assert [p[0] for p in sc.PAIRINGS] == ["side_side", "default_side"]


def test_the_classes_match_the_library_source():
    """an `ordered` or `synchronising` entry point enters the stream (ENTER_STREAM, directly or through the body it forwards to); a
    `launch_only` one does not, and its body names no engine buffer"""
    src = ""
    csrc = os.path.join(ROOT, "mbrl-lib_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith(".hip"):
            with open(os.path.join(csrc, name)) as fh:
                src += fh.read()
    bodies = {}
    for m in re.finditer(r"^int (hipets_\w+)\(", src, re.M):
        end = src.index("\n}\n", m.start())
        bodies[m.group(1)] = src[m.start():end]
    impl = {m.group(1): src[m.start():src.index("\n}\n", m.start())] for m in re.finditer(r"^int (\w+_impl|set_model)\(", src, re.M)}

    def enters(symbol, depth=0):
        body = bodies[symbol]
        if "ENTER_STREAM(" in body:
            return True
        called = [n for n in re.findall(r"\b(hipets_\w+|\w+_impl(?:<\w+>)?|set_model)\(", body) if n != symbol]
        for n in called:
            n = re.sub(r"<\w+>", "", n)
            if n in impl and "ENTER_STREAM(" in impl[n]:
                return True
            if n in bodies and depth < 2 and enters(n, depth + 1):
                return True
        return False

    engine_buffers = re.findall(r"^\s*(?:DevBuf|hipets::MlpSnapshot|hipets::EnsembleSnapshot) ([^;]+);", open(os.path.join(csrc, "engine.hpp")).read(), re.M)
    names = {n.strip() for decl in engine_buffers for n in decl.split(",")}
    assert {"totals", "population", "sac_ws", "train_slab", "policy", "ensemble"} <= names
    for symbol in sc.ORDERED.keys() | set(sc.SYNCHRONISING) | set(sc.NEEDS_COMMUNICATOR):
        assert enters(symbol), f"{symbol} is classed as taking part in the ordering, but its body never enters the stream"
    for symbol in sc.SYNCHRONISING:
        body = bodies[symbol] + "".join(impl[n] for n in impl if re.search(rf"\b{n}\(", bodies[symbol]))
        assert "hipStreamSynchronize(st)" in body, f"{symbol} is classed as synchronising"
    for symbol in sc.LAUNCH_ONLY:
        body = bodies[symbol]
        assert "ENTER_STREAM(" not in body, f"{symbol} is classed launch_only but enters the stream"
        used = sorted(n for n in names if re.search(rf"\be->{n}\b", body))
        assert not used, f"{symbol} is classed launch_only but uses the engine's {used}"


def test_the_gpu_chains_are_generated_from_this_table():
    import test_gpu_streams as gs

    assert gs.CHAINS is sc.CHAINS
    steps = {s for chain in sc.CHAINS.values() for s in chain}
    assert set(gs.STEPS) == steps, f"steps without a function: {sorted(steps - set(gs.STEPS))}; functions without a step: {sorted(set(gs.STEPS) - steps)}"
    assert set(gs.FAMILY) == set(sc.CHAINS) and set(gs.PLAN_MODE) <= set(sc.CHAINS)
    assert gs.PAIRING_IDS == [p[0] for p in sc.PAIRINGS]
    # the module names no ordered symbol in a call of its chains: a step's function gets Engine._call bound to the step's own symbol
    with open(gs.__file__) as fh:
        text = fh.read()
    chain_part = text[text.index("STEPS = {}"):text.index("# running a chain")]
    literal = set(re.findall(r"_call\(\s*\"(hipets_\w+)\"", chain_part)) | set(re.findall(r"_call, \"(hipets_\w+)\"", chain_part))
    assert literal <= {"hipets_policy_set", "hipets_critic_set"}, literal  # (the resets that put a snapshot back before the gate)
    # the parametrisation: every chain in both pairings
    marks = [m for m in gs.test_gated_chain_gives_the_serial_bits.pytestmark if m.name == "parametrize"]
    assert {m.args[0]: list(m.args[1]) for m in marks} == {"chain": list(sc.CHAINS), "pairing": gs.PAIRING_IDS}


def test_the_header_and_the_integration_guide_state_the_table():
    with open(os.path.join(ROOT, "include", "hipets.h")) as fh:
        header = fh.read()
    conventions = header[header.index("Conventions"):header.index("#ifndef HIPETS_H")]
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        guide = fh.read()
    for symbol in sc.LAUNCH_ONLY + sc.SYNCHRONISING:
        assert symbol in conventions, f"the Conventions paragraph of hipets.h does not name {symbol}"
        assert symbol.replace("hipets_", "") in guide[guide.index("## Streams"):], f"INTEGRATION.md's streams paragraph does not name {symbol}"
    assert "#define HIPETS_ABI_VERSION 9" in header
