# Builds tests/_build/inflate_print: the rules of device/zmx_inflate.h as a plain C++ program (inflate_print.cc).
# SANITIZE="-fsanitize=address,undefined" SUFFIX=_san builds it with sanitizers under another name.
ROOT := $(abspath ../..)
DEV  := $(ROOT)/zopfli_amd/csrc/device
OUT  := $(ROOT)/tests/_build
SUFFIX ?=

all: $(OUT)/inflate_print$(SUFFIX)
.PHONY: all

$(OUT)/inflate_print$(SUFFIX): inflate_print.cc $(DEV)/zmx_inflate.h
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(DEV) -o $@ inflate_print.cc
