# Builds tests/_build/png_lodeflate_print: the rules of device/zmx_png_lodeflate.h and host/png_lodeflate_size.h as a
# plain C++ program (png_lodeflate_print.cc).
# SANITIZE="-fsanitize=address,undefined" SUFFIX=_san builds it with sanitizers under another name.
ROOT := $(abspath ../..)
DEV  := $(ROOT)/zopfli_amd/csrc/device
HOST := $(ROOT)/zopfli_amd/csrc/host
OUT  := $(ROOT)/tests/_build
SUFFIX ?=

all: $(OUT)/png_lodeflate_print$(SUFFIX)
.PHONY: all

$(OUT)/png_lodeflate_print$(SUFFIX): png_lodeflate_print.cc $(DEV)/zmx_png_lodeflate.h $(HOST)/png_lodeflate_size.h
	mkdir -p $(OUT)
	g++ -O2 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(DEV) -I$(HOST) -o $@ png_lodeflate_print.cc
