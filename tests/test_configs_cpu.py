"""CPU: every section of every file under configs/ builds through the registries (model, optimizer, scheduler,
SWA optimizer / scheduler, dataset.train / val / test on generated folders), the shipped configs equal the
reference's files (their sections stored in tests/golden/ref_configs.json), and the schedules follow the reference's formulas."""
import glob
import math
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

from conftest import reference_configs
import rs_detection_amd.data  # noqa: F401
import rs_detection_amd.models  # noqa: F401
from rs_detection_amd.config import Config
from rs_detection_amd.optims import lr_scheduler, optimizer  # noqa: F401
from rs_detection_amd.utils.registry import DATASETS, MODELS, OPTIMS, SCHEDULERS, TRANSFORMS, build_from_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = sorted(glob.glob(os.path.join(ROOT, "configs", "*", "*.py")))
REF = ["s2anet_r50_fpn_1x_dota.py", "s2anet_r101_fpn_1x_dota_rotate_balance_ms.py", "orcnn_van3_7_anchor.py"]


def _make_folder(tmp_path, n=3, size=64):
    """A DOTA-format folder (images/ + labels.pkl) so that dataset sections with a ``dataset_dir`` can be built."""
    from PIL import Image
    d = tmp_path / "set"
    (d / "images").mkdir(parents=True)
    infos, rng = [], np.random.default_rng(0)
    for i in range(n):
        Image.fromarray(rng.integers(0, 255, (size, size, 3), dtype=np.uint8)).save(d / "images" / ("%d.png" % i))
        infos.append(dict(filename="%d.png" % i, width=size, height=size,
                          ann=dict(bboxes=np.array([[32, 32, 20, 10, 0.3], [10, 12, 0.5, 0.5, 0.0]], np.float32),
                                   labels=np.array([1 + i % 3, 2], np.int32),
                                   bboxes_ignore=np.zeros((0, 5), np.float32), labels_ignore=np.zeros((0,), np.int32))))
    with open(d / "labels.pkl", "wb") as f:
        pickle.dump(infos, f)
    return str(d)


def test_config_list_covers_the_baseline_configs():
    names = {os.path.basename(c) for c in CONFIGS}
    assert {"retinanet_hbb_r50_fpn.py", "s2anet_r50_fpn_1x_dota.py", "orcnn_van3_7_anchor.py",
            "s2anet_r101_fpn_1x_dota_rotate_balance_ms.py"} <= names


@pytest.mark.parametrize("path", CONFIGS, ids=[os.path.basename(c) for c in CONFIGS])
def test_every_section_builds(path, tmp_path):
    cfg = Config(path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # pretrained=True has no file offline (tested below)
        model = build_from_cfg(cfg.model, MODELS)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = build_from_cfg(cfg.optimizer, OPTIMS, params=params)
    sch = build_from_cfg(cfg.scheduler, SCHEDULERS, optimizer=opt)
    assert sch is None or callable(sch.step)
    if cfg.optimizer_swa:
        swa = build_from_cfg(cfg.optimizer_swa, OPTIMS, params=params)
        ssch = build_from_cfg(cfg.scheduler_swa, SCHEDULERS, optimizer=swa)
        base = swa.cur_lr()
        ssch.step(0.5)
        assert swa.cur_lr() == pytest.approx(cfg.scheduler_swa["min_lr"] + 0.5 * (base - cfg.scheduler_swa["min_lr"]))
    folder = _make_folder(tmp_path)
    for name, sec in (cfg.dataset or {}).items():
        sec = dict(sec)
        if "dataset_dir" in sec:
            sec["dataset_dir"] = folder
        if "images_dir" in sec:
            sec["images_dir"] = os.path.join(folder, "images")
        sec["batch_size"] = min(int(sec.get("batch_size", 1)), 2)
        if sec["type"] == "SyntheticDOTADataset":
            sec.update(tile=64, num_images=4)
        ds = build_from_cfg(sec, DATASETS)
        ds.set_shard(0, 1)
        images, targets = next(iter(ds))
        assert images.ndim == 4 and images.shape[1] == 3 and len(targets) == images.shape[0]
        if name != "test":
            assert all(t["rboxes"].shape[1] == 5 for t in targets)


@pytest.mark.parametrize("name", sorted(REF))
def test_shipped_configs_equal_the_reference(name):
    mine = Config([c for c in CONFIGS if os.path.basename(c) == name][0]).dump()
    theirs = reference_configs()[name]
    keys = ["model", "optimizer", "scheduler", "max_epoch", "log_interval", "checkpoint_interval"]
    if name.startswith("orcnn"):
        keys += ["optimizer_swa", "scheduler_swa", "swa_start_epoch", "eval_interval", "merge_nms_threshold_type"]
    if "r101" in name:
        keys += ["dataset", "eval_interval", "dataset_root"]     # this one keeps the reference's dataset section too
    for k in keys:
        assert mine.get(k) == theirs.get(k), k


def test_fair1m_dataset_drops_tiny_boxes_and_balances(tmp_path):
    folder = _make_folder(tmp_path, n=4)
    ds = build_from_cfg(dict(type="FAIR1M_1_5_Dataset", dataset_dir=folder, batch_size=1, filter_empty_gt=False), DATASETS)
    assert ds.CLASSES[0] == "Airplane" and len(ds.CLASSES) == 10
    assert all(len(i["ann"]["bboxes"]) == 1 for i in ds.img_infos)          # the 0.5 x 0.5 box (area <= 1) is gone
    bal = build_from_cfg(dict(type="FAIR1M_1_5_Dataset", dataset_dir=folder, balance_category=True), DATASETS)
    # labels 1,2,3,1 -> Airplane x1 (2 images), Ship x2 (1 image), Vehicle x1 (1 image)
    assert len(bal) == 2 * 1 + 1 * 2 + 1 * 1


def test_cosine_annealing_matches_the_reference_formula():
    p = [torch.nn.Parameter(torch.zeros(1))]
    opt = build_from_cfg(dict(type="AdamW", lr=1e-4, weight_decay=0.05), OPTIMS, params=p)
    sch = build_from_cfg(dict(type="CosineAnnealingLR", min_lr=1e-6), SCHEDULERS, optimizer=opt)
    for f in (0.0, 0.25, 0.5, 0.999):
        sch.step(f)
        assert opt.cur_lr() == pytest.approx(1e-6 + 0.5 * (1e-4 - 1e-6) * (math.cos(math.pi * f) + 1))
    sch2 = build_from_cfg(dict(type="CosineAnnealingLR", min_lr_ratio=0.1), SCHEDULERS, optimizer=opt)
    sch2.step(1.0)
    assert opt.cur_lr() == pytest.approx(0.1 * sch2.base_lr)


def test_pretrained_request_without_a_file_warns_loudly(tmp_path, monkeypatch):
    from rs_detection_amd.utils.registry import BACKBONES
    monkeypatch.delenv("RSDET_PRETRAINED_DIR", raising=False)
    with pytest.warns(RuntimeWarning, match="RANDOM"):
        m = build_from_cfg(dict(type="Resnet18", pretrained=True), BACKBONES)
    # ... and loads by name when a file is there
    from rs_detection_amd.runner.checkpoint import save_checkpoint
    torch.nn.init.constant_(m.conv1.weight, 0.25)
    save_checkpoint(str(tmp_path / "resnet18.pkl"), m)
    monkeypatch.setenv("RSDET_PRETRAINED_DIR", str(tmp_path))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m2 = build_from_cfg(dict(type="Resnet18", pretrained=True), BACKBONES)
    assert float(m2.conv1.weight.mean()) == 0.25 and len(m2.pretrained_report[0]) > 50


def test_indices_refuse_a_dataset_smaller_than_one_global_batch(tmp_path):
    folder = _make_folder(tmp_path, n=3)
    ds = build_from_cfg(dict(type="DOTADataset", dataset_dir=folder, batch_size=2), DATASETS)
    ds.set_shard(0, 2)
    with pytest.raises(ValueError, match="cannot fill"):
        ds._indices()
    ds.set_shard(1, 2, keep_all=True)              # evaluation sharding: every image once, unequal counts allowed
    assert list(ds._indices()) == [1]
    big = build_from_cfg(dict(type="SyntheticDOTADataset", tile=32, batch_size=2, num_images=9), DATASETS)
    big.set_shard(1, 2)
    assert list(big._indices()) == [1, 3, 5, 7]    # 9 -> 8 = two whole global batches of 4
