from .datasets import (ArrayDataset, bigram_successor, load_text_split, mask_dataset_static, synthetic_bigram,
                       synthetic_classification, synthetic_mlm, synthetic_mlm_raw, tokenize_dataset)
from .loader import BatchLoader
from .packing import pack_batch, position_rule, unpack_rows
from .tokenization import Tokenizer, load_tokenizer

__all__ = ["ArrayDataset", "synthetic_classification", "synthetic_mlm", "synthetic_mlm_raw", "synthetic_bigram",
           "bigram_successor", "mask_dataset_static", "load_text_split", "tokenize_dataset",
           "BatchLoader", "Tokenizer", "load_tokenizer", "pack_batch", "position_rule", "unpack_rows"]
