"""T5Embedder: prompts -> (caption features, attention mask), the shape of the reference's call (diffusion/model/t5.py:90-111)."""
import torch

from .encoder import T5Encoder


class T5Embedder:
    """encoder: a T5Encoder on the GPU (any callable (input_ids, attention_mask) -> (B, L, d_model) will do); tokenizer: any callable with the transformers
    tokenizer call signature returning 'input_ids' and 'attention_mask'.

    The reference cleans captions first (T5Embedder.clean_caption, which needs ftfy and bs4); that text cleaning is OUT OF SCOPE here: texts are
    tokenised as given, so pass cleaned (or at least lower-cased, stripped) captions."""

    def __init__(self, encoder, tokenizer, model_max_length=120):
        self.encoder, self.tokenizer, self.model_max_length = encoder, tokenizer, int(model_max_length)

    @classmethod
    def from_pretrained(cls, path, device="cuda", model_max_length=120, tokenizer_path=None, weight_dtype=None):
        """T5Encoder.from_pretrained(path) plus the tokenizer of the same directory; transformers is imported here, and only for the tokenizer.
        weight_dtype: None (as stored: an FP8 directory gives an FP8 encoder) or "fp8_e4m3" (quantise a 16-bit checkpoint while loading)."""
        from transformers import AutoTokenizer
        return cls(T5Encoder.from_pretrained(path, device=device, weight_dtype=weight_dtype), AutoTokenizer.from_pretrained(tokenizer_path or path), model_max_length)

    def get_text_embeddings(self, texts):
        tok = self.tokenizer(texts, max_length=self.model_max_length, padding="max_length", truncation=True, return_attention_mask=True,
                             add_special_tokens=True, return_tensors="pt")
        ids = torch.as_tensor(tok["input_ids"])[:, :self.model_max_length]
        mask = torch.as_tensor(tok["attention_mask"])[:, :self.model_max_length]
        with torch.no_grad():
            embs = self.encoder(ids, mask)
        return embs, mask.to(embs.device)
