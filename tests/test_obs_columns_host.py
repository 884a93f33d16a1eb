"""The parametric observation preprocessing (hipets.ObsColumns; include/hipets.h HIPETS_OBS_COLUMNS) on the host, no GPU: the
callable restates the two preprocessors mbrl.env ships (against the oracle, which is bitwise the reference) on torch tensors and
numpy arrays, the class and ModelSpec.validate refuse what the kernels cannot take, spec_from_model_env recognises an instance,
and the ctypes binding has the header's new entry point without a new ABI version.  (What hipets_set_model_columns itself refuses
needs an engine: tests/test_gpu_obs_columns.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import hipets
from conftest import ROOT
from hipets import ObsColumn, ObsColumns, UnsupportedModelError
from hipets import _lib
from oracle import pets_oracle as po


def halfcheetah_columns(obs_dim=18):
    """HalfCheetahEnv.preprocess_fn (pets_halfcheetah.py:91-113): [s1, sin s2, cos s2, s3:]"""
    return ObsColumns([(1, "id"), (2, "sin"), (2, "cos")] + [(d, "id") for d in range(3, obs_dim)])


def cartpole_pets_columns(obs_dim=4):
    """CartPoleEnv.preprocess_fn (pets_cartpole.py:78-101): [sin s1, cos s1, s0, s2:]"""
    return ObsColumns([(1, "sin"), (1, "cos"), (0, "id")] + [(d, "id") for d in range(2, obs_dim)])


RESTATED = {"halfcheetah": (18, halfcheetah_columns, po.obs_halfcheetah), "cartpole_pets": (4, cartpole_pets_columns, po.obs_cartpole_pets)}


@pytest.mark.parametrize("name", sorted(RESTATED))
def test_tables_restate_the_shipped_preprocessors_bit_for_bit(name):
    obs, make, ref_fn = RESTATED[name]
    table = make(obs)
    g = torch.Generator().manual_seed(0)
    s = torch.randn(258, obs, generator=g) * 3.0  # (256 finite rows)
    s[5, 1] = float("nan")
    s[9, 2 if name == "halfcheetah" else 1] = float("inf")
    ref = ref_fn(s)
    got = table(s)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.isnan(ref[9]).any()  # sin(inf) is NaN
    assert torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(ref, nan=7.0))
    fin = torch.isfinite(s).all(-1)
    assert torch.equal(table(s[fin]), ref_fn(s[fin]))
    assert torch.equal(table(s[3]), ref_fn(s[3]))  # 1-D: one observation (ModelEnv.reset / the agent's act)
    assert torch.equal(table(s[fin].view(2, -1, obs)[:, :100]), ref_fn(s[fin].view(2, -1, obs)[:, :100]))  # any leading shape, not contiguous
    # float64 and numpy input (Normalizer.update feeds numpy arrays: one_dim_tr_model.py update_normalizer): dtype preserved
    d = s[fin].double()
    assert table(d).dtype == torch.float64 and torch.equal(table(d), ref_fn(d))
    for arr in (s[fin].numpy(), d.numpy(), s[3].numpy()):
        out = table(arr)
        assert isinstance(out, np.ndarray) and out.dtype == arr.dtype
        assert np.array_equal(out, ref_fn(torch.from_numpy(arr)).numpy())
    assert not np.shares_memory(table(s[3].numpy()), s[3].numpy())
    before = s.clone()
    table(s)
    assert torch.equal(torch.nan_to_num(s), torch.nan_to_num(before))  # the input is never written


def test_a_table_no_shipped_form_covers():
    table = ObsColumns([(3, "cos"), (0, "id"), (1, "sin"), (1, "cos"), (2, "id"), (3, "sin"), (1, "id"), (0, "cos")])  # dim 4 unused, dim 1 three times
    assert table.columns[0] == ObsColumn(3, "cos") and table.columns[1] == ObsColumn(0)  # tuples become columns; fn defaults to id
    s = torch.randn(11, 5, generator=torch.Generator().manual_seed(1))
    ref = torch.stack([s[:, 3].cos(), s[:, 0], s[:, 1].sin(), s[:, 1].cos(), s[:, 2], s[:, 3].sin(), s[:, 1], s[:, 0].cos()], dim=1)
    assert torch.equal(table(s), ref)
    assert table == ObsColumns([ObsColumn(*c) for c in [(3, "cos"), (0, "id"), (1, "sin"), (1, "cos"), (2, "id"), (3, "sin"), (1, "id"), (0, "cos")]])
    hash(table)  # frozen: usable as a key, comparable by value


@pytest.mark.parametrize("cols, obs_dim, match", [
    ([], None, "0 columns"),
    ([(0, "id")] * 513, None, "513 columns"),
    ([(0, "id"), (-1, "sin")], None, "column 1: dim -1 outside [0, obs_dim)"),
    ([(0, "id"), (1, "id"), (5, "cos")], 5, "column 2: dim 5 outside [0, 5)"),
    ([(0, "id"), (1.5, "id")], None, "column 1: dim 1.5"),
    ([(0, "tan")], None, "column 0: fn 'tan'"),
    ([(0, "id"), (1, "id"), (2, "id"), (3, "SIN")], None, "column 3: fn 'SIN'"),
])
def test_validate_names_the_column_it_refuses(cols, obs_dim, match):
    with pytest.raises(UnsupportedModelError, match=re.escape(match)):
        if obs_dim is None:
            ObsColumns(cols)
        else:
            ObsColumns(cols).validate(obs_dim)


def small_spec(n_cols=None, **kw):
    E, obs, act, hid = 3, 5, 2, 8
    n_in = (obs if n_cols is None else n_cols) + act
    d = dict(weights=[torch.zeros(E, n_in, hid), torch.zeros(E, hid, hid), torch.zeros(E, hid, 2 * obs)],
             biases=[torch.zeros(E, 1, hid), torch.zeros(E, 1, hid), torch.zeros(E, 1, 2 * obs)],
             obs_dim=obs, act_dim=act, min_logvar=-10 * torch.ones(1, obs), max_logvar=0.5 * torch.ones(1, obs))
    d.update(kw)
    return hipets.ModelSpec(**d)


TABLE8 = ObsColumns([(3, "cos"), (0, "id"), (1, "sin"), (1, "cos"), (2, "id"), (3, "sin"), (1, "id"), (0, "cos")])


def test_model_spec_takes_a_table_and_checks_the_input_width():
    small_spec(8, obs_process=TABLE8).validate()  # wider than obs_dim
    small_spec(3, obs_process=ObsColumns([(4, "sin"), (4, "cos"), (0, "id")])).validate()  # narrower
    with pytest.raises(UnsupportedModelError, match=re.escape("model in_size 7 != obs'+act = 10")):
        small_spec(obs_process=TABLE8).validate()
    with pytest.raises(UnsupportedModelError, match=re.escape("column 1: dim 5 outside [0, 5)")):
        small_spec(2, obs_process=ObsColumns([(0, "id"), (5, "sin")])).validate()
    # names are checked exactly as before
    with pytest.raises(UnsupportedModelError, match="obs_process_fn 'acrobot' has no fused implementation"):
        small_spec(obs_process="acrobot").validate()
    small_spec(6, obs_process="cartpole_pets").validate()


# ---- spec_from_model_env / spec_from_checkpoint ---------------------------------------------------------------------------------
class _Lin:
    def __init__(self, w, b):
        self.weight, self.bias, self.use_bias = torch.nn.Parameter(w), torch.nn.Parameter(b), True


class _FakeModelEnv:
    """the attributes spec_from_model_env reads from a live mbrl.models.ModelEnv"""

    def __init__(self, obs_process_fn, n_cols):
        s = small_spec(n_cols)

        class Obj:
            pass

        mlp = Obj()
        mlp.hidden_layers = [[_Lin(w, b), torch.nn.SiLU()] for w, b in zip(s.weights[:-1], s.biases[:-1])]
        mlp.mean_and_logvar = _Lin(s.weights[-1], s.biases[-1])
        mlp.min_logvar, mlp.max_logvar = s.min_logvar, s.max_logvar
        mlp.elite_models, mlp.propagation_method, mlp.deterministic = None, "random_model", False
        dm = Obj()
        dm.model, dm.input_normalizer, dm.obs_process_fn = mlp, None, obs_process_fn
        dm.target_is_delta, dm.no_delta_list, dm.learned_rewards = True, [], False
        self.dynamics_model = dm
        self.reward_fn = lambda a, o: o[:, :1]
        self.reward_fn.hipets_closed_form = "halfcheetah"
        self.termination_fn = lambda a, o: torch.zeros(len(o), 1, dtype=torch.bool)
        self.termination_fn.hipets_closed_form = "no_termination"
        self.observation_space, self.action_space = Obj(), Obj()
        self.observation_space.shape, self.action_space.shape = (5,), (2,)


def test_spec_from_model_env_recognises_an_instance_and_nothing_else():
    spec = hipets.spec_from_model_env(_FakeModelEnv(TABLE8, 8))
    assert spec.obs_process is TABLE8 and spec.in_dim == 10
    assert hipets.spec_from_model_env(_FakeModelEnv(None, None)).obs_process == "none"
    # ... and still validates what it recognised: dims against the model, the width against the first layer
    with pytest.raises(UnsupportedModelError, match=re.escape("column 0: dim 6 outside [0, 5)")):
        hipets.spec_from_model_env(_FakeModelEnv(ObsColumns([(6, "sin")] * 8), 8))
    with pytest.raises(UnsupportedModelError, match="in_size"):
        hipets.spec_from_model_env(_FakeModelEnv(TABLE8, 7))
    # an arbitrary callable keeps its error, and learns about the class
    with pytest.raises(UnsupportedModelError, match="obs_process_fn") as exc:
        hipets.spec_from_model_env(_FakeModelEnv(lambda s: torch.cat([s, s[..., :3].sin()], -1), 8))
    assert "has no fused implementation" in str(exc.value) and "hipets.ObsColumns" in str(exc.value)
    tagged = lambda s: s  # noqa: E731
    tagged.hipets_closed_form = "acrobot"
    with pytest.raises(UnsupportedModelError, match="has no fused implementation"):
        hipets.spec_from_model_env(_FakeModelEnv(tagged, None))


def test_spec_from_checkpoint_takes_a_table_where_it_takes_a_name(tmp_path):
    s = small_spec(8)
    sd = {f"hidden_layers.{i}.0.weight": w for i, w in enumerate(s.weights[:-1])}
    sd.update({f"hidden_layers.{i}.0.bias": b for i, b in enumerate(s.biases[:-1])})
    sd.update({"mean_and_logvar.weight": s.weights[-1], "mean_and_logvar.bias": s.biases[-1], "min_logvar": s.min_logvar, "max_logvar": s.max_logvar})
    torch.save({"state_dict": sd, "elite_models": None}, tmp_path / "model.pth")
    spec = hipets.spec_from_checkpoint(tmp_path, 5, 2, obs_process=TABLE8)
    assert spec.obs_process is TABLE8 and spec.in_dim == 10
    with pytest.raises(UnsupportedModelError, match="in_size"):
        hipets.spec_from_checkpoint(tmp_path, 5, 2, obs_process="none")


# ---- header / binding -----------------------------------------------------------------------------------------------------------
def test_the_new_entry_point_comes_without_a_new_abi_version():
    assert _lib.ABI_VERSION == 9
    header = open(os.path.join(ROOT, "include", "hipets.h")).read()
    assert re.search(r"#define HIPETS_ABI_VERSION 9\b", header)
    assert ctypes.sizeof(_lib.ObsColumnC) == 8

    def fields(struct_name):
        body = re.search(r"typedef struct \{([^{}]*)\} " + struct_name + ";", header, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.findall(r"([a-z_0-9]+)\s*$", decl.strip())[0] for decl in body.split(";") if decl.strip()]

    assert fields("hipets_obs_column") == [f[0] for f in _lib.ObsColumnC._fields_] == ["dim", "fn"]
    for name, value in (("HIPETS_OBS_COLUMNS", _lib.OBS["columns"]), ("HIPETS_MAX_OBS_COLUMNS", _lib.MAX_OBS_COLUMNS),
                        ("HIPETS_COL_ID", _lib.COL_FN["id"]), ("HIPETS_COL_SIN", _lib.COL_FN["sin"]), ("HIPETS_COL_COS", _lib.COL_FN["cos"])):
        assert int(re.search(name + r"\s*=?\s*(\d+)", header).group(1)) == value, name
    assert _lib.OBS["columns"] == 3 and _lib.MAX_OBS_COLUMNS == 512
    assert tuple(_lib.COL_FN) == hipets.model.COL_FNS
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"int hipets_set_model_columns\(hipets_engine\* e, const hipets_model_desc\* desc, const hipets_obs_column\* cols, int32_t n_cols, void\* stream\);", plain)
    assert "hipets_set_model_columns" in _lib.SYMBOLS
    res, args = _lib.SYMBOLS["hipets_set_model_columns"]
    assert res is ctypes.c_int and args[1:4] == [("desc", ctypes.POINTER(_lib.ModelDesc)), ("cols", ctypes.POINTER(_lib.ObsColumnC)),
                                                 ("n_cols", ctypes.c_int32)]
    # the descriptor has not changed: the fields and the size it had (what tests/test_reward_terms_host.py pins, restated)
    assert [f[0] for f in _lib.ModelDesc._fields_][-7:] == ["reward_terms", "term_intervals", "n_reward_terms", "n_term_intervals", "reward_bias", "alive_bonus",
                                                          "term_require_finite"]
    assert hasattr(_lib.load(), "hipets_set_model_columns")
