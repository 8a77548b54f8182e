"""Three scenes with 0, 2 and 5 kept boxes: the inputs of tests/golden/tiny_pipeline_scene_boxes.pt (tools/make_golden.py sceneboxes) and of
tests/test_scene_boxes*.py.  Per scene the BATCH-1 form: boxes padded to the scene's own count (None without a kept box), as a one-scene call of
the reference gets them from collate_samples; `batched` pads them to one length, as a call that holds all three does."""
import numpy as np
import torch

from magicdrive_amd import synthetic

COUNTS = (0, 2, 5)
SEEDS = (4100, 4200, 4500)
STEPS, GUIDANCE = 5, 2.0
HW = (28, 50)


def _boxes(seed, k, n_cam=6):
    """synthetic.boxes draws a random prefix length per camera: reseed until one camera keeps all k, so the scene's padded length is k."""
    while True:
        b = synthetic.boxes(torch.Generator().manual_seed(seed), n_cam, k)
        if b["masks"][:, -1].any():
            return {key: v.unsqueeze(0) for key, v in b.items()}
        seed += 1


def make_scenes(cfg, hw=HW):
    out = []
    for k, seed in zip(COUNTS, SEEDS):
        sc = synthetic.make_scene_batch(1, seed=seed, ctx_dim=cfg["cross_attention_dim"], max_len=None, latent_hw=hw)
        sc["bboxes_3d_data"] = _boxes(seed, k) if k else None
        out.append(sc)
    return out


def batched(scenes, L=None):
    """One call holding every scene: boxes padded to L (default: the largest count) the way the dataset pads — zeros, class -1, mask False."""
    counts = [0 if s["bboxes_3d_data"] is None else s["bboxes_3d_data"]["bboxes"].shape[2] for s in scenes]
    L = max(counts) if L is None else L
    n_cam = scenes[0]["camera_param"].shape[1]
    bb = torch.zeros(len(scenes), n_cam, L, 8, 3)
    cl = torch.full((len(scenes), n_cam, L), -1, dtype=torch.int64)
    mk = torch.zeros(len(scenes), n_cam, L, dtype=torch.bool)
    for i, (s, k) in enumerate(zip(scenes, counts)):
        if k:
            b = s["bboxes_3d_data"]
            bb[i, :, :k], cl[i, :, :k], mk[i, :, :k] = b["bboxes"][0], b["classes"][0], b["masks"][0]
    out = {key: torch.cat([s[key] for s in scenes]) for key in ("prompt_embeds", "negative_prompt_embeds", "bev_map", "camera_param", "latents")}
    out["bboxes_3d_data"] = {"bboxes": bb, "classes": cl, "masks": mk}
    return out


# the BEV map is 8 x 200 x 200 zeros and ones: stored as bits
def pack_scene(sc):
    m = sc["bev_map"]
    assert ((m == 0) | (m == 1)).all()
    out = {k: v.clone() for k, v in sc.items() if k not in ("bev_map", "bboxes_3d_data")}
    out["bev_map_bits"] = torch.from_numpy(np.packbits(m.numpy().astype(np.uint8).reshape(-1)))
    out["bev_map_shape"] = tuple(m.shape)
    out["bboxes_3d_data"] = None if sc["bboxes_3d_data"] is None else {k: v.clone() for k, v in sc["bboxes_3d_data"].items()}
    return out


def unpack_scene(p):
    shape = tuple(p["bev_map_shape"])
    bits = np.unpackbits(p["bev_map_bits"].numpy())[:int(np.prod(shape))]
    out = {k: v for k, v in p.items() if k not in ("bev_map_bits", "bev_map_shape")}
    out["bev_map"] = torch.from_numpy(bits.astype(np.float32)).reshape(shape)
    return out
