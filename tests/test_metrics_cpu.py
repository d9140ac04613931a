"""CPU side of the evaluation metrics (moss_amd.metrics, C ABI moss_eval_metrics): the torch composition against the reference's own
numbers (tests/golden/eval_metrics.npz, tests/golden/make_golden_eval.py), the C declarations and their ctypes mirror, and the MOSS-side
diff that uses them."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.test_host_cpu import _apply_exactly, _diff_hunks
from tests.helpers import c_layout, ctypes_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_metrics.npz")


def _grid(z, key):
    """The fixture's images: stored as uint8 grid indices q, the float32 values are exactly q / 128 - 0.25 (tests/golden/make_golden_eval.py)."""
    return z[key + "_q"].astype(np.float32) / np.float32(128) - np.float32(0.25)


def _sets():
    z = np.load(GOLDEN)
    return z, sorted({k.split("_")[0] for k in z.files})


def test_fixture_covers_the_cases_the_semantics_turn_on():
    z, sets = _sets()
    assert sets == ["a", "b", "c"]
    sizes = {tuple(_grid(z, f"{s}_image").shape[-2:]) for s in sets}
    assert {(97, 131), (64, 48), (256, 256)} <= sizes
    assert {float(z[f"{s}_bg"].sum()) for s in sets} == {0.0, 3.0}                         # black and white backgrounds
    kinds = set()
    for s in sets:
        for b, hb in zip(z[f"{s}_bound"], z[f"{s}_has_bound"]):
            kinds.add("none" if not hb else ("zero" if not b.any() else "partial"))
        assert _grid(z, f"{s}_image").min() < 0 and _grid(z, f"{s}_image").max() > 1 and _grid(z, f"{s}_gt").min() < 0 and _grid(z, f"{s}_gt").max() > 1
    assert kinds == {"none", "zero", "partial"}
    assert max(len(z[f"{s}_l1"]) for s in sets) >= 5
    assert np.isinf(z["c_psnr"]).sum() == 1


@pytest.mark.parametrize("s", ["a", "b", "c"])
def test_quality_torch_reproduces_the_reference_numbers(s):
    """quality_torch (float32, CPU) == train_ZJU.py:244-253 composed of the reference's own l1_loss / psnr / ssim, per view."""
    from moss_amd.metrics import quality_torch
    z = np.load(GOLDEN)
    bg = torch.from_numpy(z[f"{s}_bg"])
    acc = [0.0, 0.0, 0.0]
    for i in range(len(z[f"{s}_l1"])):
        bound = torch.from_numpy(z[f"{s}_bound"][i]) if z[f"{s}_has_bound"][i] else None
        l1, p, ss = quality_torch(torch.from_numpy(_grid(z, f"{s}_image")[i]), torch.from_numpy(_grid(z, f"{s}_gt")[i]), bound, bg)
        assert l1.dtype == p.dtype == ss.dtype == torch.float32
        assert abs(l1.item() - z[f"{s}_l1"][i]) < 1e-6, (s, i)
        assert abs(ss.item() - z[f"{s}_ssim"][i]) < 1e-6, (s, i)
        want = float(z[f"{s}_psnr"][i])
        if math.isinf(want):
            assert math.isinf(p.item()) and p.item() > 0, (s, i, p.item())           # an exact match: +inf, as torch gives it
        else:
            assert abs(p.item() - want) < 1e-4, (s, i, p.item(), want)
        for k, v in enumerate((l1, p, ss)):
            acc[k] += v.double().item()
    n = len(z[f"{s}_l1"])
    for k, name in enumerate(("l1", "psnr", "ssim")):
        want = float(z[f"{s}_mean_{name}"])
        assert (math.isinf(want) and acc[k] / n == want) or abs(acc[k] / n - want) < (1e-4 if name == "psnr" else 1e-6)


def test_fill_goes_onto_the_render_only_and_after_the_clamp():
    from moss_amd.metrics import quality_torch
    g = torch.Generator().manual_seed(5)
    gt = torch.rand(3, 20, 24, generator=g) * 1.6 - 0.3
    image = gt.clone()
    mask = torch.zeros(1, 20, 24)
    mask[:, 4:15, 3:20] = 1
    for bg, fill in ((torch.zeros(3), 0.0), (torch.tensor([0.0, 0.0, 0.5]), 1.0)):
        l1, _, _ = quality_torch(image, gt, mask, bg)
        want = (gt.clamp(0, 1) - fill).abs()[:, (mask[0] != 1)].sum() / gt.numel()
        assert abs(l1.item() - want.item()) < 1e-6
    l1, p, s = quality_torch(image, gt, None, torch.ones(3))
    assert l1.item() == 0.0 and math.isinf(p.item()) and abs(s.item() - 1.0) < 1e-6


def test_psnr_is_the_mean_of_the_per_channel_psnrs():
    from moss_amd.metrics import quality_torch
    gt = torch.full((3, 8, 8), 0.5)
    image = gt.clone()
    image[0] += 0.1
    image[1] += 0.01
    image[2] += 0.001
    _, p, _ = quality_torch(image, gt, None, torch.zeros(3))
    per_channel = [20 * math.log10(1 / d) for d in (0.1, 0.01, 0.001)]
    assert abs(p.item() - sum(per_channel) / 3) < 1e-3
    assert abs(p.item() - 10 * math.log10(1 / ((0.1 ** 2 + 0.01 ** 2 + 0.001 ** 2) / 3))) > 5        # not the PSNR of the overall MSE


def test_header_declares_the_metric_entry_points(hip_lib):
    text = open(os.path.join(ROOT, "include", "moss_raster.h")).read()
    assert re.search(r"#define\s+MOSS_ABI_VERSION\s+7\b", text)
    diag = re.search(r"#ifdef MOSS_DIAG\n(.*?)#endif", text, flags=re.S).group(0)
    public = text.replace(diag, "")
    for name in ("moss_eval_metrics", "moss_metrics_workspace_bytes", "moss_metrics_state_bytes"):
        assert re.search(r"\b%s\s*\(" % name, public) and name not in diag, name
        assert hasattr(hip_lib, name), name
    assert "} moss_eval_metrics_args;" in public
    n = int(re.search(r"#define\s+MOSS_METRICS_STATE_BYTES\s+(\d+)", public).group(1))
    assert hip_lib.moss_metrics_state_bytes() == n >= 64
    # the comment cites the reference lines it implements
    block = public[public.index("Evaluation metrics of a split"):public.index("} moss_eval_metrics_args;")]
    for cite in ("train_ZJU.py:244-253", "utils/image_utils.py:19-21", "utils/loss_utils.py:41-42", "utils/loss_utils.py:47-87", "render_ZJU.py:73-94"):
        assert cite in block, cite


def test_workspace_size_is_a_host_function_of_the_shape(hip_lib):
    for B, C, H, W in ((1, 3, 97, 131), (8, 3, 1024, 1024), (8, 1, 2048, 2048), (3, 3, 33, 31)):
        tiles = ((W + 31) // 32) * ((H + 31) // 32)
        got = hip_lib.moss_metrics_workspace_bytes(B, C, H, W)
        assert got >= B * C * tiles * 3 * 4 and got % 256 == 0
    assert hip_lib.moss_metrics_workspace_bytes(0, 3, 8, 8) == 0


def test_ctypes_struct_matches_the_c_layout(tmp_path):
    """moss_amd._lib.EvalMetricsArgs mirrors moss_eval_metrics_args field by field (compiled against the header with the host compiler)."""
    from moss_amd._lib import EvalMetricsArgs
    fields = [f[0] for f in EvalMetricsArgs._fields_]
    assert c_layout(tmp_path, "moss_eval_metrics_args", fields) == ctypes_layout(EvalMetricsArgs)


def test_report_refuses_a_cpu_device(hip_lib):
    from moss_amd.metrics import QualityReport
    with pytest.raises(RuntimeError, match="GPU"):
        QualityReport("cpu", 3, 16, 16, torch.zeros(3))


def test_eval_metrics_diff_applies_after_the_loss_diffs():
    """patches/train_ZJU_eval_metrics.diff applies hunk-exactly after train_ZJU.diff and train_ZJU_one_call_loss.diff (the documented
    order), replaces the report's metric lines by a QualityReport per split, and keeps the LPIPS call and the tensorboard writes."""
    files = {}
    for name in ("train_ZJU.diff", "train_ZJU_one_call_loss.diff", "train_ZJU_eval_metrics.diff"):
        target, hunks = _diff_hunks(os.path.join(ROOT, "patches", name))
        try:
            files[target] = _apply_exactly(files.get(target, []), hunks)
        except AssertionError as e:
            raise AssertionError(f"{name} does not apply to {target}: {e}") from None
    assert set(files) == {"train_ZJU.py"}
    src = "\n".join(s for s in files["train_ZJU.py"] if s is not None)
    assert "from moss_amd.metrics import QualityReport" in src
    assert 'report = QualityReport("cuda", *config[\'cameras\'][0].original_image.shape, renderArgs[1])' in src
    assert "viewpoint.moss_region = ViewRegion(viewpoint.bound_mask.cuda())" in src
    assert "report.add(" in src and "out_image=image" in src and "report.sums()" in src
    assert "lpips_test += loss_fn_vgg(image, gt_image).mean().double()" in src
    assert "tb_writer.add_images(" in src and "l1_test /= len(config['cameras'])" in src      # (the log and the writes after it read these)
    for gone in ("psnr_test += psnr(image, gt_image)", "ssim_test += ssim(image, gt_image)", "l1_test += l1_loss(image, gt_image)",
                 "renderArgs[1].sum().item()"):
        assert gone not in src, gone
    readme = open(os.path.join(ROOT, "patches", "README.md")).read()
    assert "train_ZJU_eval_metrics.diff" in readme
    assert "train_ZJU_eval_metrics.diff" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
