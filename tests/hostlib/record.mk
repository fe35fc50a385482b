# Builds tests/_build/record_print: the match record of device/zmx_record.h as a plain C++ program (record_print.cc).
# SANITIZE="-fsanitize=address,undefined" OUT_NAME=record_print_san builds it with sanitizers under another name.
ROOT := $(abspath ../..)
DEV  := $(ROOT)/zopfli_amd/csrc/device
OUT  := $(ROOT)/tests/_build
OUT_NAME ?= record_print

$(OUT)/$(OUT_NAME): record_print.cc $(DEV)/zmx_record.h
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra $(SANITIZE) -I$(DEV) -o $@ record_print.cc
