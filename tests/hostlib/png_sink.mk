# Builds tests/_build/png_sink_print: the rules of device/zmx_png_unpack.h and host/png_sink.h as a plain C++ program
# (png_sink_print.cc).
# SANITIZE="-fsanitize=address,undefined" SUFFIX=_san builds it with sanitizers under another name.
ROOT := $(abspath ../..)
DEV  := $(ROOT)/zopfli_amd/csrc/device
HOST := $(ROOT)/zopfli_amd/csrc/host
OUT  := $(ROOT)/tests/_build
SUFFIX ?=

all: $(OUT)/png_sink_print$(SUFFIX)
.PHONY: all

$(OUT)/png_sink_print$(SUFFIX): png_sink_print.cc $(DEV)/zmx_png_unpack.h $(DEV)/zmx_png_pack.h $(DEV)/zmx_png_decode.h $(DEV)/zmx_png_color.h \
		$(HOST)/png_sink.h $(HOST)/png_source.h $(HOST)/entry_checks.h
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(ROOT)/include -I$(DEV) -I$(HOST) -o $@ png_sink_print.cc
