# Builds tests/_build/png_decode_print: the rules of device/zmx_png_decode.h and host/png_decode_plan.h as a plain C++
# program (png_decode_print.cc).
# SANITIZE="-fsanitize=address,undefined" SUFFIX=_san builds it with sanitizers under another name.
ROOT := $(abspath ../..)
DEV  := $(ROOT)/zopfli_amd/csrc/device
HOST := $(ROOT)/zopfli_amd/csrc/host
OUT  := $(ROOT)/tests/_build
SUFFIX ?=

all: $(OUT)/png_decode_print$(SUFFIX)
.PHONY: all

$(OUT)/png_decode_print$(SUFFIX): png_decode_print.cc $(DEV)/zmx_png_decode.h $(DEV)/zmx_inflate.h $(HOST)/png_decode_plan.h \
                                   $(HOST)/inflate_plan.h $(HOST)/entry_checks.h $(ROOT)/include/zopfli_amd.h
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(ROOT)/include -I$(DEV) -I$(HOST) -o $@ png_decode_print.cc
