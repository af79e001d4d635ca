"""The two classifier evaluators of the unlearning pipelines over ``resnet.ResNet`` and csrc/classify.hip:

``classifier_evaluation``  DDPM/classifier_evaluation.py: a fine-tuned ResNet-34 over a folder of samples at 224 px -> average entropy,
                           average probability and accuracy of the forgotten class, and the row of results/.../result.csv.
``imageclassify``          SD/eval-scripts/imageclassify.py: ResNet-50 over the generated pictures -> top-k classes and scores per
                           ``case_number``, joined with the prompts file.

Decoding happens on the host (Pillow); the resize runs on the GPU through ``resample.resample_tables`` / ``image_resample_u8`` (Pillow's
bilinear filter bit for bit), ToTensor + Normalize inside the stem's patch kernel, softmax / entropy / top-k in sfron_classify_metrics.
The CSV files are written with the standard library in the layout pandas writes; pandas is not a dependency.

One deliberate difference: the reference's entropy ``-(p * log p).sum()`` is NaN as soon as one probability underflows to 0; here such a
term counts as 0, its limit.
"""
import csv
import io
import os
import pathlib

import numpy as np
import torch
from PIL import Image

from . import _lib, resample
from ._lib import check, ptr, stream_ptr

IMAGE_EXTENSIONS = {"bmp", "jpg", "jpeg", "pgm", "png", "ppm", "tif", "tiff", "webp"}
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
RESULT_COLUMNS = ("entropy", "prob of forgotten class", "accuracy of forgotten class")


def image_paths(folder):
    """The file list of ImagePathDataset (classifier_evaluation.py:67-77): ``*.ext`` for every image extension, sorted as paths."""
    path = pathlib.Path(folder)
    return sorted([file for ext in IMAGE_EXTENSIONS for file in path.glob("*.{}".format(ext))])


# ------------------------------------------------------------------------------------------------ loading
def resize_tables(w, h, resize, crop=None, interpolation="bilinear"):
    """(tx, ty) of the output window of a w x h image.  ``resize`` = (height, width): both axes resized independently
    (torchvision ``Resize((h, w))``), no crop.  ``resize`` = int: the short side becomes ``resize`` (``resample.resized_size``), then the
    ``crop`` x ``crop`` centre window (default: ``resize``)."""
    name = resample._filter_name(interpolation)
    if isinstance(resize, (tuple, list)):
        if crop is not None:
            raise ValueError("crop goes with an int resize")
        oh, ow = int(resize[0]), int(resize[1])
        return resample.resample_tables(w, ow, name), resample.resample_tables(h, oh, name)
    return resample.window_tables(w, h, int(resize), name, crop=crop)


def transform_host(img, resize, crop=None, interpolation="bilinear"):
    """The same transform with Pillow on the host, uint8 [H, W, 3]: the yardstick of ``load_images_u8``."""
    img = img.convert("RGB")
    if isinstance(resize, (tuple, list)):
        out = img.resize((int(resize[1]), int(resize[0])), resample._PIL_FILTER[resample._filter_name(interpolation)])
        return np.array(out, dtype=np.uint8)
    return resample.sd_transform(img, int(resize), interpolation, crop=crop)


def load_images_u8(paths, resize, crop=None, interpolation="bilinear", device="cuda"):
    """Open (``.convert("RGB")``), resize and crop the files -> device uint8 [B, H, W, 3].  Decoding on the host, one upload, the resize on
    the GPU (two launches per image), bit-identical to Pillow's."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.SfronError("load_images_u8 needs a GPU (transform_host is the host route)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    arrays, total = [], 0
    for p in paths:
        with Image.open(p) as im:
            a = np.asarray(im.convert("RGB"), dtype=np.uint8)
        arrays.append((a, total))
        total += (a.size + 15) // 16 * 16
    if not arrays:
        raise ValueError("load_images_u8: no files")
    if isinstance(resize, (tuple, list)):
        oh, ow = int(resize[0]), int(resize[1])
    else:
        oh = ow = int(resize if crop is None else crop)
    out = torch.empty(len(arrays), oh, ow, 3, dtype=torch.uint8, device=dev)
    st = resample._staging.setdefault(dev, resample._Staging(dev))
    host = st.host_bytes(total).numpy()
    for a, off in arrays:
        host[off:off + a.size] = a.reshape(-1)
    src = st.upload(total)
    for i, (a, off) in enumerate(arrays):
        h, w = a.shape[:2]
        tx, ty = resize_tables(w, h, resize, crop, interpolation)
        y0, y1 = ty.rows()
        tmp = st.tmp_bytes((y1 - y0) * ow * 3)
        check(resample.image_resample_u8(src[off:off + a.size], h, w, tx, ty, tmp, out[i], tmp_bytes=(y1 - y0) * ow * 3), "image_resample_u8")
    return out


# ------------------------------------------------------------------------------------------------ metrics
def classify_metrics(logits, target=0, topk=0, want_probs=False):
    """sfron_classify_metrics over fp32 logits [B, n_cls] on the device -> dict of device tensors: entropy [B], p_target [B], argmax [B]
    (int32), topk_p / topk_i [B, topk], probs [B, n_cls] (when asked)."""
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise ValueError("classify_metrics takes fp32 [B, n_cls] logits")
    logits = logits.contiguous()
    B, n = logits.shape
    dev = logits.device
    out = {"entropy": torch.empty(B, dtype=torch.float32, device=dev), "p_target": torch.empty(B, dtype=torch.float32, device=dev),
           "argmax": torch.empty(B, dtype=torch.int32, device=dev)}
    if topk:
        out["topk_p"] = torch.empty(B, topk, dtype=torch.float32, device=dev)
        out["topk_i"] = torch.empty(B, topk, dtype=torch.int32, device=dev)
    if want_probs:
        out["probs"] = torch.empty(B, n, dtype=torch.float32, device=dev)
    check(_lib.lib().sfron_classify_metrics(ptr(logits), n, B, n, int(target), int(topk), ptr(out.get("probs")), ptr(out["entropy"]),
                                            ptr(out["p_target"]), ptr(out["argmax"]), ptr(out.get("topk_p")), ptr(out.get("topk_i")),
                                            stream_ptr()), "classify_metrics")
    return out


# ------------------------------------------------------------------------------------------------ DDPM: classifier_evaluation.py
def _fmt(v):
    return repr(float(v))


def update_result_csv(csv_path, name, result):
    """Insert or update row ``name`` of the results table in the layout pandas writes (classifier_evaluation.py:43-64: read_csv(index_col=0),
    concat or ``df.at``, to_csv): a header whose first cell is empty, one row per name.  Cells this call does not set keep their text."""
    header, rows = [""], []
    if os.path.isfile(csv_path):
        with open(csv_path, newline="") as f:
            table = list(csv.reader(f))
        if table:
            header, rows = table[0], [r + [""] * (len(table[0]) - len(r)) for r in table[1:]]
    for col in result:
        if col not in header[1:]:
            header.append(col)
            for r in rows:
                r.append("")
    row = next((r for r in rows if r[0] == name), None)
    if row is None:
        row = [name] + [""] * (len(header) - 1)
        rows.append(row)
    for col, v in result.items():
        row[1 + header[1:].index(col)] = _fmt(v)
    buf = io.StringIO()
    wr = csv.writer(buf, lineterminator="\n")
    wr.writerow(header)
    wr.writerows(rows)
    d = os.path.dirname(csv_path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(csv_path, "w", newline="") as f:
        f.write(buf.getvalue())
    return buf.getvalue()


def evaluate_logit_batches(batches, n_samples, label_of_forgotten_class=0):
    """The arithmetic of ``validate`` (classifier_evaluation.py:16-40) over an iterable of device logit batches: per-batch sums divided by
    ``n_samples`` -- the entropy and probability sums leave the device per batch and add up in double, the accuracy adds up in fp32."""
    entropy_cum_sum, forgotten_prob_cum_sum, accuracy_cum_sum = 0, 0, None
    for logits in batches:
        m = classify_metrics(logits, target=label_of_forgotten_class)
        accuracy = (m["argmax"] == label_of_forgotten_class).sum() / n_samples
        accuracy_cum_sum = accuracy if accuracy_cum_sum is None else accuracy_cum_sum + accuracy
        entropy_cum_sum += (torch.sum(m["entropy"]) / n_samples).item()
        forgotten_prob_cum_sum += (m["p_target"] / n_samples).sum().item()
    return {"entropy": float(entropy_cum_sum), "prob of forgotten class": float(forgotten_prob_cum_sum),
            "accuracy of forgotten class": float(accuracy_cum_sum.cpu()) if accuracy_cum_sum is not None else 0.0}


def classifier_evaluation(model, sample_path, label_of_forgotten_class=0, batch_size=64, img_size=224, csv_path=None):
    """DDPM/classifier_evaluation.py: ``model`` (a loaded ``resnet.ResNet``) over every image of ``sample_path`` at img_size x img_size,
    bytes normalised with 0.5 / 0.5.  With ``csv_path`` the row ``sample_path.split("/")[-4] + "/" + [-3]`` is inserted or updated."""
    files = image_paths(sample_path)
    n = len(files)
    if n == 0:
        raise FileNotFoundError(f"{sample_path}: no image files")

    def batches():
        for lo in range(0, n, batch_size):
            imgs = load_images_u8(files[lo:lo + batch_size], (img_size, img_size), device=model.dev)
            yield model.forward_u8(imgs, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))

    result = evaluate_logit_batches(batches(), n, label_of_forgotten_class)
    if csv_path is not None:
        parts = sample_path.split("/")
        update_result_csv(csv_path, parts[-4] + "/" + parts[-3], result)
    return result


# ------------------------------------------------------------------------------------------------ SD: imageclassify.py
def case_number(name):
    """imageclassify.py:94-100."""
    return int(name.split("/")[-1].split("_")[0].replace(".png", "").replace(".jpg", ""))


def join_prompts(prompts_path, results, save_path=None):
    """``pd.merge(read_csv(prompts_path), DataFrame(results)).to_csv(save_path)`` with the standard library: the inner join on
    ``case_number`` in the prompts file's row order, a running index in the first column.  ``results``: {column: list}, ``case_number``
    among them.  Returns (header, rows); cells of the prompts file keep their text."""
    with open(prompts_path, newline="") as f:
        table = list(csv.reader(f))
    head, body = table[0], table[1:]
    ci = head.index("case_number")
    cols = [c for c in results if c != "case_number"]
    by_case = {}
    for k, c in enumerate(results["case_number"]):
        by_case.setdefault(int(c), []).append(k)
    header = [""] + head + cols
    rows = []
    for r in body:
        if not r:
            continue
        case = int(float(r[ci]))
        for k in by_case.get(case, ()):
            left = list(r)
            left[ci] = str(case)
            rows.append([str(len(rows))] + left + [str(results[c][k]) for c in cols])
    if save_path is not None:
        with open(save_path, "w", newline="") as f:
            wr = csv.writer(f, lineterminator="\n")
            wr.writerow(header)
            wr.writerows(rows)
    return header, rows


def imageclassify(model, folder_path, prompts_path, save_path=None, topk=5, batch_size=250, categories=None):
    """SD/eval-scripts/imageclassify.py: ``model`` (a loaded ResNet-50) over the ``.png`` / ``.jpg`` files of ``folder_path`` (sorted) with the
    preprocessing of ``ResNet50_Weights.DEFAULT.transforms()`` (bilinear resize to 232, centre crop 224, ImageNet mean / std); writes the
    prompts file joined on ``case_number`` with category_topK / index_topK / scores_topK to ``save_path`` (default
    ``{folder}/{folder name}_classification.csv``).  ``categories``: the class names by index (None: the index stands in).  Returns the
    results dict {column: list}."""
    if save_path is None:
        name_ = folder_path.split("/")[-1]
        save_path = f"{folder_path}/{name_}_classification.csv"
    names = sorted(n for n in os.listdir(folder_path) if ".png" in n or ".jpg" in n)
    if not names:
        raise FileNotFoundError(f"{folder_path}: no .png / .jpg files")
    if batch_size is None or batch_size > len(names):
        batch_size = len(names)
    probs, ids = [], []
    for lo in range(0, len(names), batch_size):
        imgs = load_images_u8([os.path.join(folder_path, n) for n in names[lo:lo + batch_size]], 232, crop=224, device=model.dev)
        m = classify_metrics(model.forward_u8(imgs, IMAGENET_MEAN, IMAGENET_STD), topk=topk)
        probs.append(m["topk_p"].cpu().numpy())
        ids.append(m["topk_i"].cpu().numpy())
    probs, ids = np.concatenate(probs), np.concatenate(ids)
    results = {"case_number": [case_number(n) for n in names]}
    for k in range(1, topk + 1):
        idx = [int(i) for i in ids[:, k - 1]]
        results[f"category_top{k}"] = [categories[i] if categories is not None else i for i in idx]
        results[f"index_top{k}"] = idx
        results[f"scores_top{k}"] = list(probs[:, k - 1])
    join_prompts(prompts_path, results, save_path)
    return results
