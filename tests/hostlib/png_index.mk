# Builds tests/_build/png_index_print: the rules of device/zmx_png_index.h and host/png_index.h as a plain C++ program
# (png_index_print.cc).
# SANITIZE="-fsanitize=address,undefined" SUFFIX=_san builds it with sanitizers under another name.
ROOT := $(abspath ../..)
DEV  := $(ROOT)/zopfli_amd/csrc/device
HOST := $(ROOT)/zopfli_amd/csrc/host
OUT  := $(ROOT)/tests/_build
SUFFIX ?=

all: $(OUT)/png_index_print$(SUFFIX)
.PHONY: all

$(OUT)/png_index_print$(SUFFIX): png_index_print.cc $(DEV)/zmx_png_index.h $(DEV)/zmx_png_color.h $(HOST)/png_index.h $(HOST)/png_color_choose.h
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(ROOT)/include -I$(DEV) -I$(HOST) -o $@ png_index_print.cc
