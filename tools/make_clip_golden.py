"""Regenerates tests/golden/clip_text_tiny.pt (CPU, needs transformers): a tiny CLIPTextModel with seeded weights, bf16-rounded, three id
rows with EOS / pad tails of different lengths, and transformers' own fp32 last_hidden_state on them.

    python tools/make_clip_golden.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(vocab_size=64, hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
            max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5)


def main():
    import transformers
    torch.manual_seed(20)
    cfg = transformers.CLIPTextConfig(**TINY, bos_token_id=62, eos_token_id=63, pad_token_id=63)
    model = transformers.CLIPTextModel(cfg).eval().float()
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    g = torch.Generator().manual_seed(21)
    ids = torch.full((3, 77), 63, dtype=torch.int64)                # EOS doubles as the pad token (SD-1.5's tokenizer)
    for row, n in enumerate((5, 40, 75)):                           # BOS, n words, EOS, pad tail
        ids[row, 0] = 62
        ids[row, 1:1 + n] = torch.randint(0, 62, (n,), generator=g)
    with torch.no_grad():
        out = model(input_ids=ids).last_hidden_state.float()
    sd = {k: v.detach().to(torch.bfloat16) for k, v in model.state_dict().items() if not k.endswith("position_ids")}
    path = os.path.join(ROOT, "tests", "golden", "clip_text_tiny.pt")
    torch.save({"config": TINY, "state_dict": sd, "input_ids": ids, "last_hidden_state": out, "transformers": transformers.__version__}, path)
    print(path, os.path.getsize(path), "bytes; keys", list(sd)[:3], "...")


if __name__ == "__main__":
    sys.exit(main())
