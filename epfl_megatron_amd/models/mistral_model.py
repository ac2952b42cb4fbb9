"""Mistral-7B: Llama-2 layers with GQA, sliding-window attention
(``--sliding_window_size``) and a configurable RoPE base (``--rope_theta``):
GPTModel + flag checks."""
import torch

from .. import global_vars
from .gpt_model import GPTModel
from .llama_model import _ADVISED, _REQUIRED as _LLAMA_REQUIRED, check_rules

_REQUIRED = [(pred, msg.replace("Llama", "Mistral")) for pred, msg in _LLAMA_REQUIRED] + [
    # the fused scale-mask-softmax kernel of the non-flash GPU path knows the
    # plain causal mask only; the window runs in the FlashAttention kernels or
    # through the CPU path's boolean mask
    (lambda a: not getattr(a, "sliding_window_size", None) or a.use_flash_attn
     or getattr(a, "distributed_backend", None) == "gloo" or not torch.cuda.is_available(),
     "Mistral's sliding window needs --use_flash_attn (or the CPU path)"),
]
_ADVISED = [(pred, msg.replace("Llama", "Mistral")) for pred, msg in _ADVISED]


class MistralModel(GPTModel):
    def __init__(self, num_tokentypes=0, parallel_output=True, pre_process=True,
                 post_process=True, model_type=None):
        check_rules(global_vars.get_args(), _REQUIRED, _ADVISED)
        super().__init__(num_tokentypes=num_tokentypes, parallel_output=parallel_output,
                         pre_process=pre_process, post_process=post_process,
                         model_type=model_type)
