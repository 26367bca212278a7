"""GPU: the dataset reader feeding the device -- loader workers -> pinned staging -> the device half of the input transform
-> the tiny model's training step and ``engine.inference`` -- over the seven-image dataset of tests/tiny_coco.py."""
import copy
import random

import pytest
import torch

from tests import tiny_coco

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return tiny_coco.write(tmp_path_factory.mktemp("tiny_coco"))


@pytest.fixture(scope="module")
def cfg():
    return tiny_coco.small_cfg()


@pytest.fixture(scope="module")
def train_set(cfg, paths):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.datasets import COCOCapDetDataset

    # the five images with a usable annotation: every batch can be trained on
    return COCOCapDetDataset(paths["instances"], paths["captions"], paths["img_dir"], True, extra_args=cfg.DATASETS.DATASET_ARGS,
                             vocab_file=paths["vocab"])


def _by_hand(dataset, transform, idx, seed, epoch):
    """The batch of dataset items ``idx`` from the decoded arrays: host half, plain copies, device half."""
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import batch_seed

    items = [dataset[i] for i in idx]
    raw, targets = transform.host([it[0] for it in items], [it[1] for it in items], rng=random.Random(batch_seed(seed, 0, idx[0], epoch)))
    host = transform.device(raw)  # the host-tensor side of _C.transform_images
    dev = transform.device({k: v.cuda() if torch.is_tensor(v) else v for k, v in raw.items()})
    return host, dev, [t.to("cuda") for t in targets]


def _through_the_prefetcher(loader, transform):
    """-> (the device batches, ``raw["loader"]`` of each as the prefetcher handed it to the transform)."""
    from cvpr22_cross_modal_pseudo_labeling_amd.data.prefetch import DevicePrefetcher

    report = []

    def spy(batch):
        report.append(batch[0]["loader"])
        return transform(batch)

    stream = DevicePrefetcher(loader, "cuda", depth=2, transform=spy)
    try:
        return list(stream), report
    finally:
        stream.close()


def test_loader_workers_to_device_batches(cfg, train_set):
    """num_workers=2 -> DevicePrefetcher(transform=) -> the device: every ImageList is bit-equal to ``_C.transform_images`` on
    the host tensors of the same batch, the targets arrive on the device with their PolygonMasks intact, and no worker
    process had the GPU initialised -- although the process that forked them has."""
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import make_data_loader
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import ImageList, PolygonMasks

    torch.zeros(1, device="cuda")
    assert torch.cuda.is_initialized()
    transform = build_transforms(cfg, is_train=True)
    loader = make_data_loader(cfg, train_set, transform, True, 0, 1, num_workers=2, seed=5, max_iter=6)
    got, report = _through_the_prefetcher(loader, transform)
    assert len(got) == 6 and len(report) == 6
    assert {r["worker"] for r in report} == {0, 1} and [r["cuda_initialized"] for r in report] == [False] * 6
    for (images, targets), r in zip(got, report):
        host, dev, want_targets = _by_hand(train_set, transform, r["indices"], 5, r["epoch"])
        assert isinstance(images, ImageList) and images.tensors.is_cuda and images.tensors.dtype == torch.float32
        assert images.image_sizes == host.image_sizes and torch.equal(images.tensors.cpu(), host.tensors)
        assert torch.equal(images.tensors, dev.tensors)
        tiny_coco.assert_same_targets(targets, want_targets)
        for t in targets:
            m = t.get_field("masks")
            assert t.bbox.is_cuda and t.get_field("labels").is_cuda and t.get_field("ids_cap").is_cuda
            assert isinstance(m, PolygonMasks) and m.coords.is_cuda and len(m) == len(t) and m.size == t.size
            assert isinstance(t.get_field("caption"), str) and t.get_field("is_det") == "Yes"


def test_one_training_step_on_a_loader_batch_equals_the_hand_built_batch(cfg, train_set):
    """One optimisation step of the tiny student-teacher model on the loader's first batch and on the same batch built by hand
    from the decoded arrays, both from the same initial weights: finite, bit-equal losses and bit-equal updated weights."""
    from tests.tiny_model import build_tiny
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import make_data_loader
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import comm, solver, trainer

    model, e_vocab, _, _, _ = build_tiny("student_teacher_mask_rcnn_uncertainty")
    transform = build_transforms(cfg, is_train=True)
    loader = make_data_loader(cfg, train_set, transform, True, 0, 1, num_workers=2, seed=9, max_iter=1)
    ((images, targets),), (report,) = _through_the_prefetcher(loader, transform)
    idx = report["indices"]
    assert len(idx) == 2 and all(len(t) >= 1 for t in targets)
    _, by_hand, by_hand_targets = _by_hand(train_set, transform, idx, 9, report["epoch"])

    def step(images, targets):
        m = copy.deepcopy(model).cuda()
        m.set_class_embeddings(train_set.class_emb_mtx.cuda())  # the annotation file's: background + 4 classes
        m.set_caption_vocab(e_vocab.cuda())
        m.train()
        opt = solver.make_optimizer(cfg, m)
        red = comm.BucketedGradReducer(m)
        torch.manual_seed(100)
        losses = {k: float(v.detach()) for k, v in trainer.train_step(m, opt, red, images, targets).items()}
        red.remove()
        return losses, {n: p.detach().clone() for n, p in m.named_parameters() if p.requires_grad}

    l_loader, w_loader = step(images, targets)
    l_hand, w_hand = step(by_hand, by_hand_targets)
    print("losses on the loader batch:", l_loader)
    assert {"loss_classifier", "loss_box_reg", "loss_mask"} <= set(l_loader)
    assert all(v == v and abs(v) < 1e6 for v in l_loader.values()), l_loader
    assert l_loader == l_hand, (l_loader, l_hand)
    assert [n for n in w_loader if not torch.equal(w_loader[n], w_hand[n])] == []
    assert any(float((w_loader[n] - p.detach().cuda()).abs().max()) > 0 for n, p in model.named_parameters() if n in w_loader)


def test_inference_over_the_eval_loader(cfg, paths, tmp_path):
    """``engine.inference.inference`` over the evaluation loader: one BoxList per dataset image, in index order, each at the
    transformed image size, classified against the dataset's own class embeddings."""
    from tests.tiny_model import build_tiny
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import build_dataset, make_data_loader
    from cvpr22_cross_modal_pseudo_labeling_amd.data.catalog import DatasetCatalog
    from cvpr22_cross_modal_pseudo_labeling_amd.data.prefetch import DevicePrefetcher
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms, get_size
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import inference

    model = build_tiny("zeroshot_mask")[0].cuda()
    dataset = build_dataset(cfg, "coco_generalized_zeroshot_val", DatasetCatalog(paths["catalog"], paths["root"]))
    transform = build_transforms(cfg, is_train=False)
    loader = make_data_loader(cfg, dataset, transform, False, 0, 1, num_workers=2)
    stream = DevicePrefetcher(loader, "cuda", depth=2, transform=transform)
    preds = inference.inference(model, stream, "coco_generalized_zeroshot_val", "cuda", str(tmp_path),
                                class_embeddings=dataset.class_emb_mtx)
    stream.close()
    assert len(preds) == len(dataset) == 5 and (tmp_path / "predictions.pth").exists()
    for i, det in enumerate(preds):
        info = dataset.get_img_info(i)
        oh, ow = get_size(info["width"], info["height"], cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
        assert det.size == (ow, oh) and det.bbox.device.type == "cpu" and set(det.fields()) >= {"scores", "labels"}
        if len(det):
            assert float(det.bbox[:, 0::2].max()) <= ow - 1 and float(det.bbox[:, 1::2].max()) <= oh - 1
            assert 1 <= int(det.get_field("labels").min()) and int(det.get_field("labels").max()) <= 4


def test_worker_processes_never_initialise_the_gpu(cfg, train_set):
    """The worker-init hook records ``torch.cuda.is_initialized()`` of its process, the collate function reports it (and the
    state at batch time) with every batch: False in every worker, while the process that started them has the GPU open."""
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import make_data_loader
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms

    torch.zeros(1, device="cuda")
    assert torch.cuda.is_initialized()
    transform = build_transforms(cfg, is_train=True)
    reports = [raw["loader"] for raw, _ in make_data_loader(cfg, train_set, transform, True, 0, 1, num_workers=2, max_iter=4)]
    assert {r["worker"] for r in reports} == {0, 1} and [r["cuda_initialized"] for r in reports] == [False] * 4
    here = [raw["loader"] for raw, _ in make_data_loader(cfg, train_set, transform, True, 0, 1, num_workers=0, max_iter=1)]
    assert here[0]["worker"] is None and here[0]["cuda_initialized"] is True  # the report is live: this process has it open
