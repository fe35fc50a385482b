# Builds tests/_build/png_source_print: the rules of device/zmx_png_pack.h and host/png_source.h as a plain C++ program
# (png_source_print.cc).
# SANITIZE="-fsanitize=address,undefined" SUFFIX=_san builds it with sanitizers under another name.
ROOT := $(abspath ../..)
DEV  := $(ROOT)/zopfli_amd/csrc/device
HOST := $(ROOT)/zopfli_amd/csrc/host
OUT  := $(ROOT)/tests/_build
SUFFIX ?=

all: $(OUT)/png_source_print$(SUFFIX)
.PHONY: all

$(OUT)/png_source_print$(SUFFIX): png_source_print.cc $(DEV)/zmx_png_pack.h $(DEV)/zmx_png_color.h $(HOST)/png_source.h $(HOST)/entry_checks.h
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(ROOT)/include -I$(DEV) -I$(HOST) -o $@ png_source_print.cc
