from .functional import (  # noqa: F401
    add_rms_norm,
    build_rope_cache,
    layer_fusion_enabled,
    packed_rope_attention,
    packed_rope_attention_supported,
    cross_entropy,
    extension_available,
    flash_attention,
    fused_adamw,
    fused_rope,
    moe_ffn,
    moe_ffn_supported,
    moe_route,
    rms_norm,
    swiglu,
)
from . import reference  # noqa: F401
