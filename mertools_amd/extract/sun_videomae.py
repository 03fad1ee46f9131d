"""View planning and reduction of MER2024's fine-tuned VideoMAE extractor (feature_extraction/visual/extract_sun_videomae.py).

The reference's test dataset (videomae/kinetics.py: VideoClsDatasetFrame) builds test_num_segment x test_num_crop = 4 views per
item; `final_test` (videomae/engine_for_finetuning.py:11-45) averages the 4 view features of each frame id in float64.  Many of
those views are the same 16-frame window: both spatial crops of a square-resized frame coincide, all 4 FRAME views of a frame id are
one window, and the first 10 / last 9 frame ids share one window each.  A clip's features do not depend on its batch mates, so the
model only has to see each DISTINCT window once; `reduce_views` then rebuilds every frame id's 4-row block in item order and reduces it
exactly as the reference does.
"""
import numpy as np

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def item_frames(N, feature_level, clip_len=16, sampling_rate=4, test_num_segment=2, test_num_crop=2):
    """-> list of (frmid, ck, cp, [source frame numbers of the view]) in the reference's item order (kinetics.py:55-128).
    The window constants 10 / 8 / 16 / 17 are literal there (they do not follow clip_len); negative indices wrap as Python's do."""
    if N <= 0:
        raise ValueError(f"a video needs at least one frame (N={N})")
    items = []

    def load(idxs):
        idxs = list(idxs)
        while len(idxs) < clip_len:
            idxs.append(idxs[-1])
        return [min(i, N - 1) % N for i in idxs]   # frames[min(idx, N-1)]; numpy wraps a negative index once

    if feature_level == "UTTERANCE":
        buf = load(range(0, N, sampling_rate))
        tstep = max(1.0 * (len(buf) - clip_len) / (test_num_segment - 1), 0) if test_num_segment > 1 else 0
        for ck in range(test_num_segment):
            for cp in range(test_num_crop):
                t0 = int(ck * tstep)
                items.append((0, ck, cp, buf[t0:t0 + clip_len]))
    elif feature_level == "FRAME":
        for ck in range(test_num_segment):
            for cp in range(test_num_crop):
                for frmid in range(N):
                    if frmid < 10:
                        start, end = 0, 16
                    elif frmid > N - 10:
                        start, end = N - 17, N - 1
                    else:
                        start, end = frmid - 8, frmid + 8
                    assert start >= -N, (N, frmid)   # (start is -6 at worst, and only for N >= 11)
                    buf = load(range(start, end))
                    tstep = max(1.0 * (len(buf) - clip_len) / (test_num_segment - 1), 0) if test_num_segment > 1 else 0
                    t0 = int(ck * tstep)
                    items.append((frmid, ck, cp, buf[t0:t0 + clip_len]))
    else:
        raise ValueError(f"feature_level must be UTTERANCE or FRAME, not {feature_level!r}")
    return items


class ViewPlan:
    """windows int32 [U, clip_len]: the distinct views' source frame numbers; item_window int [n_items]: each reference item's window id;
    item_frmid int [n_items]: its frame id (the '%010d' key final_test groups by)."""

    def __init__(self, N, feature_level, windows, item_window, item_frmid):
        self.N, self.feature_level = N, feature_level
        self.windows, self.item_window, self.item_frmid = windows, item_window, item_frmid

    @property
    def n_items(self):
        return len(self.item_window)


def plan_views(N, feature_level, clip_len=16, sampling_rate=4, test_num_segment=2, test_num_crop=2):
    items = item_frames(N, feature_level, clip_len, sampling_rate, test_num_segment, test_num_crop)
    ids, windows, item_window = {}, [], []
    for _, _, _, fr in items:
        key = tuple(fr)
        if key not in ids:
            ids[key] = len(windows)
            windows.append(fr)
        item_window.append(ids[key])
    return ViewPlan(N, feature_level, np.asarray(windows, dtype=np.int32).reshape(-1, clip_len), np.asarray(item_window, dtype=np.int64),
                    np.asarray([it[0] for it in items], dtype=np.int64))


def reduce_items(per_item, item_frmid, feature_level):
    """final_test's reduction (engine_for_finetuning.py:28-45) of per-item features [n_items, D] (float32 rows, item order) -> the
    saved float64 array: np.mean of each frame id's rows in item order, then the squeeze rules."""
    blocks = {}
    for i, f in enumerate(item_frmid):
        blocks.setdefault("%010d" % int(f), []).append(i)
    per_item = np.asarray(per_item)
    embeddings = []
    for key in sorted(blocks):
        rows = blocks[key]
        assert len(rows) == 4, (key, len(rows))
        embeddings.append(np.mean(per_item[rows].astype(np.float64), axis=0))
    embeddings = np.array(embeddings).squeeze()
    if feature_level == "FRAME":
        if len(embeddings.shape) == 1:
            embeddings = embeddings[np.newaxis, :]
    elif len(embeddings.shape) == 2:
        embeddings = np.mean(embeddings, axis=0)
    return embeddings


def reduce_views(per_window_f32, plan):
    """Per distinct window features [U, D] -> the reference's saved array: each item takes its window's row, then reduce_items."""
    return reduce_items(np.asarray(per_window_f32)[plan.item_window], plan.item_frmid, plan.feature_level)


def host_pixels(frames_resized_u8, frame_numbers, mean=MEAN, std=STD):
    """The reference's ClipToTensor + Normalize on the host (volume_transforms.py / functional.py:76-88): resized u8 frames
    [n, S, S, 3] (BGR as stored: no channel swap) and one view's frame numbers -> float32 [3, T, S, S]:
    (float32(u) / 255 - mean[c]) / std[c], true division, float32 throughout."""
    import torch
    buf = np.asarray(frames_resized_u8)[np.asarray(frame_numbers)]
    t = torch.from_numpy(buf.transpose(3, 0, 1, 2).astype(np.float64)).float()
    t = torch.div(t, 255)
    m = torch.as_tensor(mean, dtype=torch.float32)
    s = torch.as_tensor(std, dtype=torch.float32)
    return t.sub_(m[:, None, None, None]).div_(s[:, None, None, None])


def save_dir_name(checkpoint, feature_level):
    """extract_sun_videomae.py:232-235: '{checkpoint parent dir}-{epoch}-{UTT|FRA}' ('.../videomae-base-VoxCeleb2/checkpoint-99.pth' ->
    'videomae-base-VoxCeleb2-99-UTT')."""
    import os
    model_name, epoch_name = os.path.normpath(checkpoint).replace(os.sep, "/").split("/")[-2:]
    epoch_name = epoch_name[:-4].split("-")[1]
    return f"{model_name}-{epoch_name}-{feature_level[:3]}"


def pil_resize_host(frame_u8, S):
    """Image.fromarray(frame).convert('RGB').resize((S, S), BILINEAR) (kinetics.py:126 + functional.py:resize_clip): the host oracle."""
    from PIL import Image
    return np.asarray(Image.fromarray(frame_u8).convert("RGB").resize((S, S), Image.BILINEAR))
