"""CPU: ``data.build.make_data_loader`` over the seven-image dataset of tests/tiny_coco.py, with the host-tensor side of
``_C.transform_images`` making the pixels; and the two tools' ``--dataset-catalog`` paths on MODEL.DEVICE cpu."""
import importlib.util
import os
import random

import pytest
import torch

from tests import tiny_coco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configs/coco_cap_det/student_teacher_mask_rcnn_uncertainty.yaml")


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"ovis_tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return tiny_coco.write(tmp_path_factory.mktemp("tiny_coco"))


@pytest.fixture(scope="module")
def cfg():
    return tiny_coco.small_cfg(extra=["MODEL.DEVICE", "cpu"])


@pytest.fixture(scope="module")
def train_set(cfg, paths):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import build_train_dataset
    from cvpr22_cross_modal_pseudo_labeling_amd.data.catalog import DatasetCatalog

    return build_train_dataset(cfg, DatasetCatalog(paths["catalog"], paths["root"]))


def test_build_dataset_follows_the_catalog_entry(cfg, paths, train_set):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import build_dataset
    from cvpr22_cross_modal_pseudo_labeling_amd.data.catalog import DatasetCatalog
    from cvpr22_cross_modal_pseudo_labeling_amd.data.datasets import COCOCapDetDataset, COCODataset

    assert type(train_set) is COCOCapDetDataset and len(train_set) == 7 and train_set.parser is not None
    val = build_dataset(cfg, "coco_zeroshot_val", DatasetCatalog(paths["catalog"], paths["root"]))
    assert type(val) is COCODataset and val.ids == tiny_coco.IDS_WITH_VALID_ANNOTATION
    assert tuple(val.class_emb_mtx.shape) == (5, 768)  # DATASETS.DATASET_ARGS of the yaml: BertEmb, 768


def test_train_batches_are_the_host_half_by_hand_whatever_the_workers(cfg, train_set):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import batch_seed, make_data_loader
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms

    transform = build_transforms(cfg, is_train=True)
    runs = {}
    for workers in (0, 2):
        loader = make_data_loader(cfg, train_set, transform, True, 0, 1, num_workers=workers, seed=77, max_iter=9)
        runs[workers] = list(loader)
        assert len(runs[workers]) == 9  # more than two passes over 7 images in batches of 2
    assert {b[0]["loader"]["worker"] for b in runs[0]} == {None} and {b[0]["loader"]["worker"] for b in runs[2]} == {0, 1}
    flips = set()
    for (raw0, targets0), (raw2, targets2) in zip(runs[0], runs[2]):
        idx = raw0["loader"]["indices"]
        assert idx == raw2["loader"]["indices"] and 1 <= len(idx) <= 2 and raw0["loader"]["epoch"] == raw2["loader"]["epoch"]
        items = [train_set[i] for i in idx]
        want_raw, want_targets = transform.host([it[0] for it in items], [it[1] for it in items],
                                                rng=random.Random(batch_seed(77, 0, idx[0], raw0["loader"]["epoch"])))
        for raw, targets in ((raw0, targets0), (raw2, targets2)):
            tiny_coco.assert_same_raw(raw, want_raw)
            tiny_coco.assert_same_targets(targets, want_targets)
            assert not raw["data"].is_cuda and raw["data"].dtype == torch.uint8
        flips.update(raw0["desc"][:, 5].tolist())
        tall = [train_set.get_img_info(i)["height"] >= train_set.get_img_info(i)["width"] for i in idx]
        assert len(set(tall)) == 1  # grouped by aspect ratio: one bin per batch
    assert flips == {0, 1}  # the draws are live: some images flipped, some not
    assert [b[0]["loader"]["epoch"] for b in runs[0]] == [0] * 4 + [4] * 4 + [8]  # the iteration each pass began at
    assert batch_seed(77, 0, 3, 0) != batch_seed(77, 0, 3, 4) and len({batch_seed(s, r, i, e) for s in (0, 1) for r in (0, 1)
                                                                       for i in (0, 1) for e in (0, 1)}) == 16
    seen = [i for raw, _ in runs[0][:4] for i in raw["loader"]["indices"]]
    assert sorted(seen) == list(range(7))  # the first pass (4 batches) is a permutation of the dataset
    other = list(make_data_loader(cfg, train_set, transform, True, 0, 1, num_workers=0, seed=78, max_iter=4))
    assert [b[0]["loader"]["indices"] for b in other] == [b[0]["loader"]["indices"] for b in runs[0][:4]]  # the order is the sampler's


def test_resumed_loader_continues_the_iteration_count(cfg, train_set):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import make_data_loader
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms

    transform = build_transforms(cfg, is_train=True)
    resumed = list(make_data_loader(cfg, train_set, transform, True, 0, 1, start_iter=6, num_workers=0, max_iter=9))
    assert len(resumed) == 3
    # its first pass is shuffled with the epoch seed 6 (set_epoch(start_iter)), not with that of a run from 0
    g = torch.Generator()
    g.manual_seed(6)
    assert resumed[0][0]["loader"]["indices"][0] == torch.randperm(7, generator=g).tolist()[0]


def test_two_ranks_share_an_epoch(cfg, train_set):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import make_data_loader
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms

    transform = build_transforms(cfg, is_train=True)
    g = torch.Generator()
    g.manual_seed(0)
    order = torch.randperm(7, generator=g).tolist()
    shares = []
    for rank in range(2):
        loader = make_data_loader(cfg, train_set, transform, True, rank, 2, num_workers=0, max_iter=10 ** 6)
        epoch = len(loader.batch_sampler.batch_sampler.batch_sampler)  # the batches of this rank's first pass
        it = iter(loader)
        batches = [next(it) for _ in range(epoch)]
        assert all(len(b[0]["loader"]["indices"]) == 1 for b in batches)  # SOLVER.IMS_PER_BATCH 2 over 2 ranks
        shares.append([i for b in batches for i in b[0]["loader"]["indices"]])
    # 7 images over 2 ranks: 4 each, contiguous slices of the epoch's order; the eighth is the wrap-around to its start
    assert sorted(shares[0]) == sorted(order[:4]) and sorted(shares[1]) == sorted(order[4:] + order[:1])
    assert set(shares[0]) | set(shares[1]) == set(range(7))
    assert set(shares[0]) & set(shares[1]) == {order[0]}
    assert set(shares[0]).isdisjoint(order[4:]) and len(set(order[4:])) == 3
    # no wrap-around when the world divides the set: the shares of 7 ranks are disjoint and cover it
    seven = tiny_coco.small_cfg(extra=["MODEL.DEVICE", "cpu", "SOLVER.IMS_PER_BATCH", 7])
    singles = []
    for rank in range(7):
        (raw, _), = list(make_data_loader(seven, train_set, transform, True, rank, 7, num_workers=0, max_iter=1))
        singles.append(raw["loader"]["indices"])
    assert singles == [[i] for i in order]


def test_eval_loader_yields_every_image_once_and_the_transform_applied_directly(cfg, paths):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import build_dataset, make_data_loader
    from cvpr22_cross_modal_pseudo_labeling_amd.data.catalog import DatasetCatalog
    from cvpr22_cross_modal_pseudo_labeling_amd.data.prefetch import DevicePrefetcher
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import ImageList

    dataset = build_dataset(cfg, "coco_zeroshot_val", DatasetCatalog(paths["catalog"], paths["root"]))
    transform = build_transforms(cfg, is_train=False)
    flat = tiny_coco.small_cfg(extra=["MODEL.DEVICE", "cpu", "DATALOADER.ASPECT_RATIO_GROUPING", False])
    for config, workers in ((flat, 0), (flat, 2), (cfg, 0)):
        loader = make_data_loader(config, dataset, transform, False, 0, 1, num_workers=workers)
        stream = DevicePrefetcher(loader, "cpu", transform=transform)
        got = list(stream)
        stream.close()
        ids = [i for _, _, chunk in got for i in chunk]
        assert sorted(ids) == list(range(5)) and all(t is None for _, t, _ in got)
        if config is flat:
            assert [chunk for _, _, chunk in got] == [[0, 1], [2, 3], [4]]  # sequential: index order
        for images, _, chunk in got:
            assert isinstance(images, ImageList)
            want = transform.device(transform.host([dataset[i][0] for i in chunk])[0])
            assert torch.equal(images.tensors, want.tensors) and images.image_sizes == want.image_sizes
            assert images.tensors.dtype == torch.float32 and images.tensors.shape[0] == len(chunk)
    # two ranks: contiguous slices; the sixth slot wraps around to index 0, which the gather merges by id
    per_rank = [[i for _, _, chunk in make_data_loader(flat, dataset, transform, False, r, 2, num_workers=0) for i in chunk]
                for r in range(2)]
    assert per_rank == [[0, 1, 2], [3, 4, 0]]


def test_divisibility_and_catalog_errors(cfg, paths, train_set, tmp_path):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import build_dataset, build_train_dataset, make_data_loader
    from cvpr22_cross_modal_pseudo_labeling_amd.data.catalog import DatasetCatalog
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms

    transform = build_transforms(cfg, is_train=True)
    with pytest.raises(ValueError, match=r"SOLVER.IMS_PER_BATCH \(2\) must be divisible by the number of GPUs \(3\) used"):
        make_data_loader(cfg, train_set, transform, True, 0, 3)
    with pytest.raises(ValueError, match=r"TEST.IMS_PER_BATCH \(2\) must be divisible by the number of GPUs \(3\) used"):
        make_data_loader(cfg, train_set, transform, False, 0, 3)
    catalog = DatasetCatalog(paths["catalog"], paths["root"])
    with pytest.raises(KeyError, match="lvis_v1_val"):
        build_dataset(cfg, "lvis_v1_val", catalog)
    with pytest.raises(FileNotFoundError, match="coco_cap_det_train"):
        build_train_dataset(cfg, DatasetCatalog(paths["catalog"], str(tmp_path)))
    two = tiny_coco.small_cfg(extra=["DATASETS.TRAIN", ("coco_cap_det_train", "coco_zeroshot_train")])
    with pytest.raises(NotImplementedError, match="coco_zeroshot_train"):
        build_train_dataset(two, catalog)


def test_train_net_data_source_without_and_with_the_catalog(cfg, train_set):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import TrainCollator
    from cvpr22_cross_modal_pseudo_labeling_amd.data.samplers import IterationBasedBatchSampler
    from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import RawSyntheticBatches, SyntheticBatches

    train_net = _tool("train_net")
    zero = tiny_coco.small_cfg(extra=["MODEL.DEVICE", "cpu", "DATALOADER.NUM_WORKERS", 0])
    loader, transform = train_net.make_data_source(zero, 2)
    assert type(loader.dataset) is SyntheticBatches and transform is None and loader.batch_size is None
    loader, transform = train_net.make_data_source(zero, 2, raw_input=True)
    assert type(loader.dataset) is RawSyntheticBatches and loader.dataset.transform is transform and loader.dataset.batch == 2
    loader, transform = train_net.make_data_source(zero, 2, dataset=train_set, start_iter=3, max_iter=5)
    assert loader.dataset.dataset is train_set and isinstance(loader.collate_fn, TrainCollator) and loader.collate_fn.transform is transform
    assert isinstance(loader.batch_sampler.batch_sampler, IterationBasedBatchSampler) and len(list(loader)) == 2
    assert loader.collate_fn.seed == 0
    assert train_net.make_data_source(zero, 2, dataset=train_set, max_iter=1, seed=31)[0].collate_fn.seed == 31


def test_tools_train_and_test_from_the_catalog_on_cpu(paths, tmp_path):
    """``tools/train_net.py`` for 2 iterations and ``tools/infer_net.py`` over one test set, MODEL.DEVICE cpu: a checkpoint and a
    ``predictions.pth`` with one BoxList per dataset image at the transformed size."""
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import get_size

    out = str(tmp_path / "out")
    cfg = tiny_coco.small_cfg(extra=["MODEL.DEVICE", "cpu", "DATALOADER.NUM_WORKERS", 0, "OUTPUT_DIR", out, "SOLVER.LOG_PERIOD", 1])
    history = _tool("train_net").train(cfg, 0, False, 2, 1, save_checkpoints=True, dataset_catalog=paths["catalog"],
                                       data_dir=paths["root"])
    assert history and all(torch.isfinite(torch.tensor(list(h[1].values()))).all() for h in history)
    assert os.path.isfile(os.path.join(out, "model_final.pth"))
    _tool("infer_net").main(["--config-file", YAML, "--dataset-catalog", paths["catalog"], "--data-dir", paths["root"],
                            "MODEL.DEVICE", "cpu", "DATALOADER.NUM_WORKERS", "0", "OUTPUT_DIR", out, "INPUT.MIN_SIZE_TEST", "80",
                            "INPUT.MAX_SIZE_TEST", "128", "TEST.IMS_PER_BATCH", "2", "MODEL.RPN.PRE_NMS_TOP_N_TEST", "200",
                            "MODEL.RPN.POST_NMS_TOP_N_TEST", "40", "DATASETS.TEST", "('coco_not_zeroshot_val',)"])
    preds = torch.load(os.path.join(out, "inference", "coco_not_zeroshot_val", "predictions.pth"), weights_only=False)
    sizes = {i: (w, h) for i, _, w, h, _ in tiny_coco.IMAGES}
    assert len(preds) == 5
    for image_id, det in zip(tiny_coco.IDS_WITH_VALID_ANNOTATION, preds):
        w, h = sizes[image_id]
        oh, ow = get_size(w, h, 80, 128)
        assert det.size == (ow, oh) and det.has_field("scores") and det.has_field("labels")
        labels = det.get_field("labels")
        assert labels.numel() == 0 or 1 <= int(labels.min()) <= int(labels.max()) <= 4  # the classes of the annotation file
