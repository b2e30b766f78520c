from .datasets import (ArrayDataset, answer_length_table, bigram_successor, conll_tag_list, load_text_split, mask_dataset_static,
                       read_conll, synthetic_bigram, synthetic_classification, synthetic_mlm, synthetic_mlm_raw,
                       synthetic_question_answering, synthetic_token_classification, tag_table, read_squad, tokenize_conll,
                       tokenize_dataset, tokenize_squad, multi_label_marker_table, regression_marker_table,
                       synthetic_multi_label, synthetic_regression)
from .loader import BatchLoader
from .packing import pack_batch, position_rule, unpack_rows
from .tokenization import Tokenizer, load_tokenizer

__all__ = ["ArrayDataset", "synthetic_classification", "synthetic_mlm", "synthetic_mlm_raw", "synthetic_bigram",
           "bigram_successor", "mask_dataset_static", "load_text_split", "tokenize_dataset",
           "synthetic_token_classification", "tag_table", "read_conll", "conll_tag_list", "tokenize_conll",
           "synthetic_question_answering", "answer_length_table", "read_squad", "tokenize_squad",
           "synthetic_regression", "synthetic_multi_label", "regression_marker_table", "multi_label_marker_table",
           "BatchLoader", "Tokenizer", "load_tokenizer", "pack_batch", "position_rule", "unpack_rows"]
