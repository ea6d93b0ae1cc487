"""Sweep files (wandb format) -> configurations, metric names, the threshold list and the CSV layouts of the offline sweep
drivers (asr_amd.sweep): host logic only, no GPU."""
import csv
import json
import math

import numpy as np
import pytest

import conftest  # noqa: F401  (puts the repository root on sys.path)
from asr_amd import distributed as D
from asr_amd import sweep as SW


def _grid():
    return {"method": "grid", "parameters": {"lambda_tv": {"values": [0.1, 0.2, 0.3]}, "optimizer": {"values": ["adam", "sgd"]},
                                             "num_iter": {"value": 50}}}


def test_grid_order_and_size():
    cfgs = SW.expand(_grid())
    assert len(cfgs) == 6
    # the first parameter varies slowest
    assert [(c["lambda_tv"], c["optimizer"]) for c in cfgs] == [(0.1, "adam"), (0.1, "sgd"), (0.2, "adam"), (0.2, "sgd"),
                                                                (0.3, "adam"), (0.3, "sgd")]
    assert all(c["num_iter"] == 50 for c in cfgs)


def test_grid_refuses_continuous_ranges():
    spec = {"method": "grid", "parameters": {"lambda_tv": {"min": 0.0, "max": 1.0}}}
    with pytest.raises(SW.SweepSpecError, match="grid"):
        SW.expand(spec)


def _random(**extra):
    spec = {"method": "random", "count": 20, "parameters": {
        "lambda_tv": {"min": 0.0, "max": 5.0, "distribution": "q_uniform", "q": 0.05},
        "lambda_L2": {"min": 0.0, "max": 1.0},
        "decay_steps": {"min": 20, "max": 100, "distribution": "q_uniform", "q": 20},
        "num_iter": {"min": 100, "max": 400, "distribution": "int_uniform"},
        "learning_rate": {"min": 1e-4, "max": 1e-1, "distribution": "log_uniform_values"},
        "optimizer": {"values": ["adam", "adagrad", "adadelta"]}}}
    spec.update(extra)
    return spec


def test_random_is_seeded():
    a, b = SW.expand(_random()), SW.expand(_random())
    assert a == b and len(a) == 20
    assert SW.expand(_random(seed=1234)) == a                 # 1234 is the default seed
    c = SW.expand(_random(), seed=99)
    assert c != a
    assert SW.expand(_random(seed=99)) == c                   # the file's seed and the argument's agree
    assert len(SW.expand(_random(), count=3)) == 3


def test_random_distributions():
    cfgs = SW.expand(_random(count=200))
    for c in cfgs:
        q = c["lambda_tv"] / 0.05
        assert 0.0 <= c["lambda_tv"] <= 5.0 and abs(q - round(q)) < 1e-6
        assert isinstance(c["decay_steps"], int) and c["decay_steps"] in (20, 40, 60, 80, 100)
        assert isinstance(c["num_iter"], int) and 100 <= c["num_iter"] <= 400
        assert 1e-4 <= c["learning_rate"] <= 1e-1
        assert 0.0 <= c["lambda_L2"] <= 1.0 and isinstance(c["lambda_L2"], float)    # float bounds without distribution
        assert c["optimizer"] in ("adam", "adagrad", "adadelta")
    assert len({c["lambda_tv"] for c in cfgs}) > 20
    assert {c["optimizer"] for c in cfgs} == {"adam", "adagrad", "adadelta"}
    ints = SW.expand({"method": "random", "count": 50, "parameters": {"num_iter": {"min": 1, "max": 3}}})
    assert {c["num_iter"] for c in ints} == {1, 2, 3} and all(isinstance(c["num_iter"], int) for c in ints)


def test_q_uniform_stays_inside_bounds_off_the_grid():
    spec = {"method": "random", "count": 300, "parameters": {
        "copy_dropout": {"min": 0.03, "max": 0.38, "distribution": "q_uniform", "q": 0.1}}}
    vals = {c["copy_dropout"] for c in SW.expand(spec)}
    assert vals == {0.1, 0.2, 0.3}


def test_random_needs_count():
    spec = _random()
    del spec["count"]
    with pytest.raises(SW.SweepSpecError, match="count"):
        SW.expand(spec)
    assert len(SW.expand(spec, count=2)) == 2


def test_bayes_runs_as_random_with_a_note(capsys):
    spec = _random(method="bayes")
    cfgs = SW.expand(spec)
    err = capsys.readouterr().err
    assert "bayes" in err and "random" in err and len(err.strip().splitlines()) == 1
    assert cfgs == SW.expand(_random())


def test_unknown_keys_are_refused():
    spec = {"method": "grid", "parameters": {"lambda_tv": {"value": 1.0}, "num_samples": {"value": 3},
                                             "lamda_L2": {"value": 0.1}}}
    with pytest.raises(SW.SweepSpecError) as e:
        SW.expand(spec)
    msg = str(e.value)
    assert "lamda_L2" in msg and "num_samples" in msg
    for k in SW.HYPER_DEFAULTS:
        assert k in msg


def test_defaults_merge():
    assert set(SW.HYPER_DEFAULTS) == {"lambda_df", "lambda_tv", "lambda_L2", "lambda_L1", "num_iter", "use_BTV",
                                      "copy_dropout", "optimizer", "learning_rate", "beta_1", "beta_2", "epsilon", "amsgrad",
                                      "initial_accumulator_value", "momentum", "nesterov", "lr_scheduler", "decay_steps",
                                      "decay_rate"}
    (c,) = SW.expand({"method": "grid", "parameters": {"lambda_tv": {"value": 0.3}, "amsgrad": {"value": True}}})
    expect = dict(SW.HYPER_DEFAULTS, lambda_tv=0.3, amsgrad=True)
    assert c == expect
    # sweep_script.py's defaults
    assert (c["lambda_L2"], c["num_iter"], c["learning_rate"], c["decay_steps"], c["decay_rate"], c["momentum"]) == \
        (0.11, 300, 1e-3, 50, 0.5, 0.6)
    assert SW.THRESHOLD_DEFAULTS["copy_dropout"] == 0.2 and SW.THRESHOLD_DEFAULTS["learning_rate"] == 0.1
    assert (SW.THRESHOLD_DEFAULTS["decay_steps"], SW.THRESHOLD_DEFAULTS["decay_rate"]) == (100, 0.65)


def test_metric_names_map_to_fields():
    expect = {"aug_iou_single": "aug_single", "aug_iou_multiple": "aug_bg", "standard_iou_single": "standard_single",
              "standard_iou_multiple": "standard_bg", "max_iou": "max", "mean_iou": "mean"}
    for name, field in expect.items():
        col, goal = SW.metric_of({"metric": {"name": name, "goal": "minimize"}})
        assert D.IOU_FIELDS[col] == field and goal == "minimize"
    assert SW.metric_of({}) == (D.IOU_FIELDS.index("aug_single"), "maximize")
    with pytest.raises(SW.SweepSpecError):
        SW.metric_of({"metric": {"name": "avg_aug_SR_iou"}})


def test_best_index_ties_and_nan():
    assert SW.best_index([0.5, 0.7, 0.7, float("nan")], "maximize") == 1
    assert SW.best_index([0.5, 0.2, 0.2], "minimize") == 1
    assert SW.best_index([float("nan")] * 2, "maximize") is None


def test_threshold_list_is_the_reference_list():
    expect = [0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9]
    assert SW.TH_FACTORS == expect and len(SW.TH_FACTORS) == 17


def test_threshold_csv_layout(tmp_path):
    p = tmp_path / "th_argmax_2.csv"
    SW.write_threshold_csv(p, [0.1, 0.15, 0.2], [0.5, 0.625, float("nan")])
    assert p.read_text().splitlines() == [",Th_Value,IoU", "0,0.1,0.5", "1,0.15,0.625", "2,0.2,"]


def test_sweep_csv_layout(tmp_path):
    cfgs = SW.expand(_grid())[:2]
    means = [{f: float(i) + 0.5 for f in D.IOU_FIELDS} for i in range(2)]
    p = tmp_path / "s.csv"
    SW.write_sweep_csv(p, cfgs, means, 3)
    rows = list(csv.reader(open(p)))
    assert rows[0] == ["index"] + list(SW.HYPER_DEFAULTS) + list(SW.METRICS) + ["n_valid"]
    assert len(rows) == 3 and rows[2][0] == "1" and rows[2][-1] == "3" and rows[2][-2] == "1.5"


def test_yaml_and_json_expand_identically(tmp_path):
    yaml = pytest.importorskip("yaml")
    text = """
method: random
count: 7
seed: 5
metric:
  goal: maximize
  name: aug_iou_single
parameters:
  lambda_df:
    value: 1.0
  lambda_tv:
    max: 5
    min: 0
    distribution: q_uniform
    q: 0.05
  learning_rate:
    values:
      - 1e-2
      - 1e-3
  use_BTV:
    values: [True, False]
"""
    (tmp_path / "s.yaml").write_text(text)
    spec_json = yaml.safe_load(text)
    spec_json["parameters"]["learning_rate"]["values"] = [1e-2, 1e-3]
    (tmp_path / "s.json").write_text(json.dumps(spec_json))
    a = SW.expand(SW.load_spec(tmp_path / "s.yaml"))
    b = SW.expand(SW.load_spec(tmp_path / "s.json"))
    assert a == b and len(a) == 7
    assert all(isinstance(c["learning_rate"], float) for c in a)         # YAML 1.1 reads 1e-2 as a string


def test_yaml_without_pyyaml_suggests_json(tmp_path, monkeypatch):
    import builtins
    real = builtins.__import__

    def no_yaml(name, *args, **kwargs):
        if name == "yaml":
            raise ImportError("no yaml")
        return real(name, *args, **kwargs)

    monkeypatch.setattr(builtins, "__import__", no_yaml)
    (tmp_path / "s.yaml").write_text("method: grid\n")
    with pytest.raises(SW.SweepSpecError, match="JSON"):
        SW.load_spec(tmp_path / "s.yaml")


def test_drop_mask_is_the_seeded_process_draw():
    """_seed_drop_mask gives the mask np.random.shuffle draws first after np.random.seed(1234)."""
    class Fake:
        num_aug, copy_dropout, _drop_masks = 10, 0.3, None

    f = Fake()
    f._drop_masks = {}
    SW._seed_drop_mask(f, 1234)
    state = np.random.get_state()
    try:
        np.random.seed(1234)
        mask = np.full(10, True)
        mask[:3] = False
        np.random.shuffle(mask)
    finally:
        np.random.set_state(state)
    assert list(f._drop_masks) == [3] and (f._drop_masks[3] == mask).all()
    assert not math.isnan(float(f._drop_masks[3].sum())) and f._drop_masks[3].sum() == 7
