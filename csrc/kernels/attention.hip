// Attention (forward + backward): one translation unit over the per-family files, so that
// the helpers they share (ATile, attn_impl.h) are specialised for one set of callers.
#include "attn_fwd.h"
#include "attn_bwd.h"
#include "attn_f8.h"
#include "attn_qkv.h"
