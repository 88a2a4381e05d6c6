"""MI355X-native fused cosine-similarity attention (drop-in for the hot path of
lucidrains/flash-cosine-sim-attention).  Same public names as the reference package
(flash_cosine_sim_attention/__init__.py:1)."""
from .ops import (flash_cosine_sim_attention, flash_cosine_sim_attention_local, flash_cosine_sim_attention_varlen,
                  flash_cosine_sim_attention_with_kvcache, flash_cosine_sim_attention_varlen_with_kvcache,
                  flash_cosine_sim_attention_prefill_with_kvcache,
                  flash_cosine_sim_attention_step_with_kvcache, flash_cosine_sim_attention_tree_with_kvcache,
                  flash_cosine_sim_attention_alibi_with_kvcache, flash_cosine_sim_attention_alibi,
                  kvcache_keep_accepted,
                  flash_cosine_sim_attention_with_shared_prefix, merge_attention_states,
                  flash_cosine_sim_attention_with_lse, merge_attention_states_with_grad,
                  plain_cosine_sim_attention, l2norm_tensors, FlashCosineSimAttention)
from .ext import debug

__version__ = '0.3.0'
__all__ = ['flash_cosine_sim_attention', 'flash_cosine_sim_attention_local', 'flash_cosine_sim_attention_varlen',
           'flash_cosine_sim_attention_with_kvcache', 'flash_cosine_sim_attention_varlen_with_kvcache',
           'flash_cosine_sim_attention_prefill_with_kvcache',
           'flash_cosine_sim_attention_step_with_kvcache', 'flash_cosine_sim_attention_tree_with_kvcache',
           'flash_cosine_sim_attention_alibi_with_kvcache', 'flash_cosine_sim_attention_alibi',
           'kvcache_keep_accepted',
           'flash_cosine_sim_attention_with_shared_prefix', 'merge_attention_states',
           'flash_cosine_sim_attention_with_lse', 'merge_attention_states_with_grad',
           'plain_cosine_sim_attention', 'l2norm_tensors', 'debug', 'FlashCosineSimAttention']
