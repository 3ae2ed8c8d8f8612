"""Reference of include/ltxhip_fp8.h on the CPU: torch's float8_e4m3fn is the format and its widening the reference's; the header's
cast SATURATES (|x| >= 448 gives +-448, NaN stays NaN) where torch's turns values beyond 464 into NaN, so the cast is restated."""
import torch

F8 = torch.float8_e4m3fn
cast = lambda x: x.float().clamp(-448.0, 448.0).to(F8)      # round to nearest even, saturating (clamp passes NaN through)
codes = lambda q: q.view(torch.uint8)
widen64 = lambda q: q.view(F8).to(torch.float64)
