#!/bin/bash
# Developer script: whisper-finetune_amd/libwft_fwdstamps.so = the library with the attention files compiled -DFWD_STAMPS (s_memtime
# sums per phase of a key tile in attn_fwd_kernel, csrc/attn_fwd.hip) for tools/dev/fwd_stamps.py.
exec make -C "$(dirname "$0")/../../whisper-finetune_amd/csrc" ATTN_DEFS=-DFWD_STAMPS OUT=../libwft_fwdstamps.so
